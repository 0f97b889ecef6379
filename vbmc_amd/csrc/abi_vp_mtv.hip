// C-ABI entry point of the marginal total variation: vbmc_vp_mtv (include/vbmc_hip.h).  The kernels are mtv_kernels.h; the draws, the
// packing of a posterior and the split of a draw are vp_tools_host.h's; the constants of fixed_point, the cosine table and the host tail
// of a column are mtv_host.h's.  Here: validation, the launches, the copies back and the sum of the integral's partials.
#include "mtv_host.h"
#include "vp_tools_host.h"

extern "C" vbmc_status vbmc_vp_mtv(vbmc_ctx* ctx, const vbmc_vp_desc* vp1, const vbmc_vp_desc* vp2, const vbmc_mtv_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_mtv";
  if (!args || args->struct_size != sizeof(vbmc_mtv_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const long long Ns = args->Ns;
  if (Ns < 2 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 2 .. %lld", who, Ns, VPT_MAXN);
  const int n = args->nkde == 0 ? 8192 : args->nkde, nquad = args->nquad == 0 ? 100000 : args->nquad;
  if (n < 256 || n > 16384 || (n & (n - 1)) != 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: nkde = %d is not a power of two in 256 .. 16384", who, n);
  if (nquad < 2 || nquad > (1 << 20)) return set_err(ctx, VBMC_ERR_INVALID, "%s: nquad = %d outside 2 .. 2^20", who, nquad);
  VptPack pk[2];
  VB_TRY(vpt_pack(ctx, who, vp1, 0.0, pk[0]));
  VB_TRY(vpt_pack(ctx, who, vp2, 0.0, pk[1]));
  if (vp1->D != vp2->D) return set_err(ctx, VBMC_ERR_INVALID, "%s: the posteriors have D = %d and D = %d", who, vp1->D, vp2->D);
  const int D = vp1->D, C2 = 2 * D;
  const size_t nX = (size_t)Ns * D;
  if (nX * 8 > ((size_t)1 << 30))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Ns x D = %lld x %d doubles per posterior exceed the 1 GiB the draws may hold on the device", Ns, D);
  hipStream_t st = ctx->stream;
  const vbmc_vp_desc* vps[2] = {vp1, vp2};
  const double* blocks[2] = {args->block1, args->block2};
  double* xx[2] = {args->xx1, args->xx2};
  const double inf = std::numeric_limits<double>::infinity();

  // ---- the draws: vbmc_rnd(vp, Ns, 1, 1) (vbmc_mtv.m:32, :41), exactly vbmc_vp_rnd's rows
  VptGenHost g[2];
  TmpBuf dXX[2];
  std::vector<double> ends(4 * (size_t)C2);
  for (int s = 0; s < 2; ++s) {
    VB_TRY(vpt_gen_host(ctx, who, D, vps[s]->K, vps[s]->w, Ns, 1, args->seed + (uint64_t)s, g[s]));
    g[s].G.origflag = 1;
    VB_TRY(vpt_upload(ctx, pk[s]));
    VB_TRY(vpt_gen_upload(ctx, who, D, blocks[s], g[s]));
    HIP_TRY(ctx, dXX[s].alloc(ctx, nX * 8));
    VptDrawArgs a{};
    a.P = pk[s].P; a.G = g[s].G; a.X = dXX[s].as<double>(); a.I = nullptr;
    const dim3 grid((unsigned)((Ns + VPT_T - 1) / VPT_T));
    VPT_FOR_DT(pk[s].DT, hipLaunchKernelGGL((k_vp_draw<DT>), grid, dim3(VPT_T), 0, st, a))
    const double* tr = pk[s].P.has_tr ? pk[s].h.data() + pk[s].o_tr : nullptr;
    for (int d = 0; d < D; ++d) {
      double* e = &ends[4 * ((size_t)s * D + d)];
      e[0] = pk[s].lb[d]; e[1] = pk[s].ub[d];
      e[2] = tr ? tr[6 * pk[s].DT + d] : -inf;
      e[3] = tr ? tr[7 * pk[s].DT + d] : inf;
    }
  }
  HIP_TRY(ctx, hipGetLastError());

  // ---- mesh, counts, cosine coefficients, bandwidth, inverse transform
  const size_t nC = (size_t)C2 * n;
  std::vector<double> htab;
  mtv_cos_table(n, htab);
  TmpBuf dEnds, dCol, dNu, dCnt, dW, dTab, dT, dStat;
  HIP_TRY(ctx, dEnds.alloc(ctx, ends.size() * 8));
  HIP_TRY(ctx, dCol.alloc(ctx, (size_t)C2 * sizeof(MtvCol)));
  HIP_TRY(ctx, dNu.alloc(ctx, (size_t)C2 * sizeof(long long)));
  HIP_TRY(ctx, dCnt.alloc(ctx, nC * sizeof(int)));
  HIP_TRY(ctx, dW.alloc(ctx, 5 * nC * 8));              // initial data, a, a2, a_t, the inverse transform
  HIP_TRY(ctx, dTab.alloc(ctx, htab.size() * 8));
  HIP_TRY(ctx, dT.alloc(ctx, (size_t)C2 * 8));
  HIP_TRY(ctx, dStat.alloc(ctx, (size_t)C2 * sizeof(int)));
  double *d_x = dW.as<double>(), *d_a = d_x + nC, *d_a2 = d_a + nC, *d_at = d_a2 + nC, *d_raw = d_at + nC;
  HIP_TRY(ctx, hipMemcpyAsync(dEnds.p, ends.data(), ends.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dTab.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(dCnt.p, 0, nC * sizeof(int), st));
  {
    MtvMeshArgs a{};
    a.Ns = (int)Ns; a.D = D; a.xx[0] = dXX[0].as<double>(); a.xx[1] = dXX[1].as<double>(); a.ends = dEnds.as<double>();
    a.col = dCol.as<MtvCol>(); a.nuniq = dNu.as<long long>();
    hipLaunchKernelGGL(k_mtv_mesh, dim3(C2), dim3(MTV_T), 0, st, a);
    MtvBinArgs b{};
    b.Ns = (int)Ns; b.D = D; b.n = n; b.xx[0] = a.xx[0]; b.xx[1] = a.xx[1]; b.col = a.col; b.counts = dCnt.as<int>();
    const unsigned nbx = (unsigned)std::min<long long>((Ns + MTV_T - 1) / MTV_T, 64);
    hipLaunchKernelGGL(k_mtv_bin, dim3(nbx, C2), dim3(MTV_T), 0, st, b);
    MtvInitArgs c{};
    c.n = n; c.col = a.col; c.counts = b.counts; c.x = d_x;
    hipLaunchKernelGGL(k_mtv_init, dim3(C2), dim3(MTV_T), 0, st, c);
  }
  const size_t lds = ((size_t)n + 1) * 8;
  if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_mtv_dct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  MtvDctArgs fw{};
  fw.n = n; fw.inverse = 0; fw.tab = dTab.as<double>(); fw.in = d_x; fw.out = d_a; fw.a2 = d_a2;
  hipLaunchKernelGGL(k_mtv_dct, dim3(n / MTV_T, C2), dim3(MTV_T), lds, st, fw);
  {
    MtvRootArgs a{};
    a.n = n; a.D = D; a.col = dCol.as<MtvCol>(); a.a = d_a; a.a2 = d_a2; a.at = d_at; a.tstar = dT.as<double>(); a.status = dStat.as<int>();
    mtv_root_consts(a);
    hipLaunchKernelGGL(k_mtv_root, dim3(C2), dim3(MTV_T), 0, st, a);
  }
  MtvDctArgs bw{};
  bw.n = n; bw.inverse = 1; bw.tab = dTab.as<double>(); bw.in = d_at; bw.out = d_raw; bw.a2 = nullptr;
  hipLaunchKernelGGL(k_mtv_dct, dim3(n / MTV_T, C2), dim3(MTV_T), lds, st, bw);
  HIP_TRY(ctx, hipGetLastError());

  std::vector<double> yy(nC), mm(nC), ht(C2);
  std::vector<MtvCol> hcol(C2);
  std::vector<int> hstat(C2);
  std::vector<long long> hnu(C2);
  HIP_TRY(ctx, hipMemcpyAsync(yy.data(), d_raw, nC * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hcol.data(), dCol.p, (size_t)C2 * sizeof(MtvCol), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hstat.data(), dStat.p, (size_t)C2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hnu.data(), dNu.p, (size_t)C2 * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(ht.data(), dT.p, (size_t)C2 * 8, hipMemcpyDeviceToHost, st));
  if (args->counts) HIP_TRY(ctx, hipMemcpyAsync(args->counts, dCnt.p, nC * sizeof(int), hipMemcpyDeviceToHost, st));
  for (int s = 0; s < 2; ++s)
    if (xx[s]) HIP_TRY(ctx, hipMemcpyAsync(xx[s], dXX[s].p, nX * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int c = 0; c < C2; ++c)
    if (hstat[c] == 1)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED,
                     "posterior %d, dimension %d: the bandwidth equation has no bracket below 0.1 (the reference's fminbnd branch, kde1d.m:136-138) -- not accelerated",
                     c / D + 1, c % D + 1);

  // ---- kde1d.m:58, :62 and vbmc_mtv.m:68, :71 on the host, then the splines
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> msh(4 * (size_t)C2), geo(4 * (size_t)D), cp;
  for (int c = 0; c < C2; ++c) mtv_finish_column(hcol[c], n, yy.data() + (size_t)c * n, mm.data() + (size_t)c * n, &msh[4 * (size_t)c], cp);
  for (int d = 0; d < D; ++d) {                                                           // vbmc_mtv.m:74
    double* bb = &geo[4 * (size_t)d];
    bb[0] = msh[4 * d]; bb[1] = msh[4 * d + 2]; bb[2] = msh[4 * (D + d)]; bb[3] = msh[4 * (D + d) + 2];
    std::sort(bb, bb + 4);
  }
  if (args->mesh)
    for (int c = 0; c < C2; ++c) { args->mesh[2 * c] = hcol[c].MIN; args->mesh[2 * c + 1] = hcol[c].MAX; }
  if (args->nuniq)
    for (int c = 0; c < C2; ++c) args->nuniq[c] = hnu[c];
  if (args->tstar)
    for (int c = 0; c < C2; ++c) args->tstar[c] = ht[c];
  if (args->density) std::memcpy(args->density, yy.data(), nC * 8);
  if (!args->mtv) return VBMC_OK;

  // ---- the integral (vbmc_mtv.m:73-78)
  const int ntile = (nquad + MTV_T - 1) / MTV_T, nb = std::min(ntile, MTV_NBLK), nent = 3 * D;
  TmpBuf dS, dG, dP;
  HIP_TRY(ctx, dS.alloc(ctx, 2 * nC * 8));
  HIP_TRY(ctx, dG.alloc(ctx, (msh.size() + geo.size()) * 8));
  HIP_TRY(ctx, dP.alloc(ctx, ((size_t)nb + 1) * nent * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dS.p, yy.data(), nC * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dS.as<double>() + nC, mm.data(), nC * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dG.p, msh.data(), msh.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dG.as<double>() + msh.size(), geo.data(), geo.size() * 8, hipMemcpyHostToDevice, st));
  MtvIntArgs ia{};
  ia.n = n; ia.D = D; ia.nquad = nquad; ia.ntile = ntile; ia.msh = dG.as<double>(); ia.geo = ia.msh + msh.size();
  ia.yy = dS.as<double>(); ia.mm = ia.yy + nC; ia.partial = dP.as<double>();
  double* d_out = ia.partial + (size_t)nb * nent;
  hipLaunchKernelGGL(k_mtv_integral, dim3(nb, D), dim3(MTV_T), 0, st, ia);
  hipLaunchKernelGGL(k_vp_reduce, dim3((nent + VPT_T - 1) / VPT_T), dim3(VPT_T), 0, st, ia.partial, nb, nent, d_out);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> ho(nent);
  HIP_TRY(ctx, hipMemcpyAsync(ho.data(), d_out, (size_t)nent * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int d = 0; d < D; ++d) {
    if (hcol[d].bad || hcol[D + d].bad) { args->mtv[d] = nan; continue; }
    double v = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double b0 = geo[4 * (size_t)d + j], b1 = geo[4 * (size_t)d + j + 1];
      if (!(b1 > b0)) continue;
      const double x1 = nquad == 2 ? b1 : b0 + (b1 - b0) / (double)(nquad - 1);         // xx_range(2)
      v = v + 0.5 * ho[3 * d + j] * (x1 - b0);                                            // vbmc_mtv.m:77
    }
    args->mtv[d] = v;
  }
  return VBMC_OK;
}

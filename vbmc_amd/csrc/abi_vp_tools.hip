// C-ABI entry points of the variational-posterior tools: vbmc_vp_pdf, vbmc_vp_rnd, vbmc_vp_moments, vbmc_vp_kldiv and
// vbmc_vp_rnd_rng_dump (include/vbmc_hip.h).  The kernels are vp_tools_kernels.h; validation, the constants of a call and the upload of
// a posterior are vp_tools_host.h.  Here: the launches, and the O(D^2) tail of the moments.  vbmc_vp_mode: its refusals here, the kernel
// mode_kernels.h, the launches and the winner rule mode_host.h.
#include "mode_host.h"
#include "parity_rng.h"
#include "vp_tools_host.h"

extern "C" vbmc_status vbmc_vp_rnd_rng_dump(uint64_t seed, int64_t N, int D, int K, int balanceflag, const double* w, double* B, int64_t* perm) {
  if (N < 1 || N > VPT_MAXN || D < 1 || K < 1 || K > VBMC_LIM_K || !w || (balanceflag != 0 && balanceflag != 1)) return VBMC_ERR_INVALID;
  double ws = 0.0;
  for (int k = 0; k < K; ++k) { if (!(std::isfinite(w[k]) && w[k] >= 0.0)) return VBMC_ERR_INVALID; ws += w[k]; }
  if (!(ws > 0.0)) return VBMC_ERR_INVALID;
  VptGenHost g;
  VB_TRY(vpt_gen_host(nullptr, "vbmc_vp_rnd_rng_dump", K, w, N, balanceflag, seed, g));
  if (B)
    for (long long i = 0; i < g.G.M; ++i) {
      B[(size_t)(D + 1) * i] = slice_uniform(seed, VPT_CTR, (unsigned)i, 0u);
      for (int d = 0; d < D; ++d) B[(size_t)(1 + d) + (size_t)(D + 1) * i] = srch_normal(seed, VPT_CTR, (unsigned)i, (unsigned)d);
    }
  if (perm)
    for (long long r = 0; r < N; ++r) perm[r] = g.G.balanced ? (int64_t)vpt_perm((unsigned)r, (unsigned)g.G.M, g.G.hb, g.G.key) : r;
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_pdf(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t N, const double* X, int origflag, int logflag, int transflag, double df, double* y,
                                   double* dy) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_pdf";
  if (df != df) return set_err(ctx, VBMC_ERR_INVALID, "%s: df is not a number", who);
  if (N < 0 || N > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: N = %lld outside 0 .. %lld", who, (long long)N, VPT_MAXN);
  VptPack pk;
  VB_TRY(vpt_pack(ctx, who, vp, df, pk));
  if (dy && vpt_heavy(df)) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "the gradient of the heavy-tailed pdf is not supported (vbmc_pdf.m:82, :100)");
  if (dy && origflag && pk.P.has_tr) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "the gradient in the original space is not supported (vbmc_pdf.m:117)");
  if (N == 0) return VBMC_OK;
  if (!X || !y) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = vp->D;
  hipStream_t st = ctx->stream;
  VB_TRY(vpt_upload(ctx, pk));
  const size_t nX = (size_t)N * D;
  TmpBuf dX, dY;
  HIP_TRY(ctx, dX.alloc(ctx, nX * 8));
  HIP_TRY(ctx, dY.alloc(ctx, ((size_t)N + (dy ? nX : 0)) * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dX.p, X, nX * 8, hipMemcpyHostToDevice, st));
  VptPdfArgs a{};
  a.P = pk.P; a.N = (int)N; a.origflag = origflag ? 1 : 0; a.logflag = logflag ? 1 : 0; a.transflag = transflag ? 1 : 0;
  a.X = dX.as<double>(); a.y = dY.as<double>(); a.dy = dy ? dY.as<double>() + N : nullptr;
  const dim3 grid((unsigned)((N + VPT_T - 1) / VPT_T));
  if (dy) { VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_pdf<DT, true>), grid, dim3(VPT_T), 0, st, a)) }
  else { VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_pdf<DT, false>), grid, dim3(VPT_T), 0, st, a)) }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(y, a.y, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  if (dy) HIP_TRY(ctx, hipMemcpyAsync(dy, a.dy, nX * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_rnd(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t N, int origflag, int balanceflag, double df, uint64_t seed, const double* block,
                                   double* X, int32_t* I) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_rnd";
  if (df != df) return set_err(ctx, VBMC_ERR_INVALID, "%s: df is not a number", who);
  if (N < 0 || N > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: N = %lld outside 0 .. %lld", who, (long long)N, VPT_MAXN);
  VptPack pk;
  VB_TRY(vpt_pack(ctx, who, vp, 0.0, pk));
  if (vpt_heavy(df)) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "sampling the heavy-tailed posterior (finite df: gamrnd, vbmc_rnd.m:87) is not accelerated");
  if (balanceflag == 2) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "sampling through the Gaussian process (vbmc_rnd.m:45-49) is not accelerated");
  if (balanceflag != 0 && balanceflag != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: balanceflag %d", who, balanceflag);
  if (N == 0) return VBMC_OK;
  if (!X) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = vp->D;
  hipStream_t st = ctx->stream;
  VptGenHost g;
  VB_TRY(vpt_gen_host(ctx, who, vp->K, vp->w, N, balanceflag, seed, g));
  g.G.origflag = origflag ? 1 : 0;
  VB_TRY(vpt_upload(ctx, pk));
  VB_TRY(vpt_gen_upload(ctx, who, D, block, g));
  const size_t nX = (size_t)N * D;
  TmpBuf dX, dI;
  HIP_TRY(ctx, dX.alloc(ctx, nX * 8));
  HIP_TRY(ctx, dI.alloc(ctx, (size_t)N * sizeof(int)));
  VptDrawArgs a{};
  a.P = pk.P; a.G = g.G; a.X = dX.as<double>(); a.I = dI.as<int>();
  const dim3 grid((unsigned)((N + VPT_T - 1) / VPT_T));
  VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_draw<DT>), grid, dim3(VPT_T), 0, st, a))
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(X, a.X, nX * 8, hipMemcpyDeviceToHost, st));
  if (I) HIP_TRY(ctx, hipMemcpyAsync(I, a.I, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_moments(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t Ns, uint64_t seed, const double* block, double* mubar, double* Sigma) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_moments";
  if (Ns < 2 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 2 .. %lld", who, (long long)Ns, VPT_MAXN);
  VptPack pk;
  VB_TRY(vpt_pack(ctx, who, vp, 0.0, pk));
  if (!mubar) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = vp->D, K = vp->K, DT = pk.DT;
  hipStream_t st = ctx->stream;
  VptGenHost g;
  VB_TRY(vpt_gen_host(ctx, who, K, vp->w, Ns, 1, seed, g));
  g.G.origflag = 1;
  // the centre of the shifted sums: the image of the mixture mean
  std::vector<double> hc(DT, 0.0), ym(D, 0.0);
  double ws = 0.0;
  for (int k = 0; k < K; ++k) ws += vp->w[k];
  for (int d = 0; d < D; ++d) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += vp->w[k] * vp->mu[d + (size_t)D * k];
    ym[d] = s / ws;
  }
  vpt_host_inverse(vp, pk, ym.data(), hc.data());
  const int nent = D + D * (D + 1) / 2;
  const VptMomEntries el(nent);
  std::vector<unsigned char> he(el.L.bytes());
  {
    unsigned char *ei = el.ei.at(he.data()), *ej = el.ej.at(he.data());
    int e = 0;
    for (int d = 0; d < D; ++d, ++e) { ei[e] = (unsigned char)d; ej[e] = (unsigned char)DT; }
    for (int j = 0; j < D; ++j)
      for (int i = 0; i <= j; ++i, ++e) { ei[e] = (unsigned char)i; ej[e] = (unsigned char)j; }
  }
  const int ntile = (int)((Ns + VPT_T - 1) / VPT_T), nb = std::min(ntile, VPT_MAXBLK);
  const VptReduceBlock rl((size_t)nb * nent, nent);
  VB_TRY(vpt_upload(ctx, pk));
  VB_TRY(vpt_gen_upload(ctx, who, D, block, g));
  TmpBuf dC, dE, dP;
  HIP_TRY(ctx, dC.alloc(ctx, (size_t)DT * 8));
  HIP_TRY(ctx, dE.alloc(ctx, he.size()));
  HIP_TRY(ctx, dP.alloc(ctx, rl.L.bytes()));
  HIP_TRY(ctx, hipMemcpyAsync(dC.p, hc.data(), (size_t)DT * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dE.p, he.data(), he.size(), hipMemcpyHostToDevice, st));
  VptMomArgs a{};
  el.bind(a, dE.p);
  a.P = pk.P; a.G = g.G; a.centre = dC.as<double>(); a.nent = nent; a.ntile = ntile;
  a.partial = rl.partial.at(dP.p);
  double* d_out = rl.out.at(dP.p);
  VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_moments<DT>), dim3(nb), dim3(VPT_T), 0, st, a))
  hipLaunchKernelGGL(k_vp_reduce, dim3((nent + VPT_T - 1) / VPT_T), dim3(VPT_T), 0, st, a.partial, nb, nent, d_out);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> ho(nent);
  HIP_TRY(ctx, hipMemcpyAsync(ho.data(), d_out, (size_t)nent * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const double n = (double)Ns;
  for (int d = 0; d < D; ++d) mubar[d] = hc[d] + ho[d] / n;
  if (Sigma) {
    int e = D;
    for (int j = 0; j < D; ++j)
      for (int i = 0; i <= j; ++i, ++e) {
        const double v = (ho[e] - ho[i] * ho[j] / n) / (n - 1.0);
        Sigma[i + (size_t)D * j] = v;
        Sigma[j + (size_t)D * i] = v;
      }
  }
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_kldiv(vbmc_ctx* ctx, const vbmc_vp_desc* vp1, const vbmc_vp_desc* vp2, int64_t Ns, uint64_t seed, const double* block1,
                                     const double* block2, double* kls, double* xx1, double* xx2) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_kldiv";
  if (Ns < 1 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 1 .. %lld", who, (long long)Ns, VPT_MAXN);
  VptPack pk[2];
  VB_TRY(vpt_pack(ctx, who, vp1, 0.0, pk[0]));
  VB_TRY(vpt_pack(ctx, who, vp2, 0.0, pk[1]));
  if (!kls) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  if (vp1->D != vp2->D) return set_err(ctx, VBMC_ERR_INVALID, "%s: the posteriors have D = %d and D = %d", who, vp1->D, vp2->D);
  const int D = vp1->D, DT = pk[0].DT;
  for (int d = 0; d < D; ++d)
    if (pk[0].lb[d] != pk[1].lb[d] || pk[0].ub[d] != pk[1].ub[d])
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "the two posteriors have different bounds in variable %d: draws of one lie outside the other's support", d + 1);
  hipStream_t st = ctx->stream;
  const vbmc_vp_desc* vps[2] = {vp1, vp2};
  const double* blocks[2] = {block1, block2};
  double* xx[2] = {xx1, xx2};
  VptGenHost g[2];
  for (int s = 0; s < 2; ++s) {
    VB_TRY(vpt_gen_host(ctx, who, vps[s]->K, vps[s]->w, Ns, 1, seed + (uint64_t)s, g[s]));
    g[s].G.origflag = 1;
  }
  const int ntile = (int)((Ns + VPT_T - 1) / VPT_T), nb = std::min(ntile, VPT_MAXBLK);
  const size_t nX = (size_t)Ns * D;
  const VptReduceBlock rl(2 * (size_t)nb, 2);            // a row of nb partial sums and a total per direction
  TmpBuf dP, dXX[2];
  HIP_TRY(ctx, dP.alloc(ctx, rl.L.bytes()));
  for (int s = 0; s < 2; ++s) {
    VB_TRY(vpt_upload(ctx, pk[s]));
    VB_TRY(vpt_gen_upload(ctx, who, D, blocks[s], g[s]));
    if (xx[s]) HIP_TRY(ctx, dXX[s].alloc(ctx, nX * 8));
  }
  double* d_out = rl.out.at(dP.p);
  for (int s = 0; s < 2; ++s) {
    VptKlArgs a{};
    a.Pg = pk[s].P; a.Po = pk[1 - s].P; a.G = g[s].G; a.ntile = ntile; a.xx = xx[s] ? dXX[s].as<double>() : nullptr;
    a.partial = rl.partial.part((size_t)s * nb, nb).at(dP.p);
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_kldiv<DT>), dim3(nb), dim3(VPT_T), 0, st, a))
    hipLaunchKernelGGL(k_vp_reduce, dim3(1), dim3(VPT_T), 0, st, a.partial, nb, 1, d_out + s);
  }
  HIP_TRY(ctx, hipGetLastError());
  double ho[2];
  HIP_TRY(ctx, hipMemcpyAsync(ho, d_out, 2 * 8, hipMemcpyDeviceToHost, st));
  for (int s = 0; s < 2; ++s)
    if (xx[s]) HIP_TRY(ctx, hipMemcpyAsync(xx[s], dXX[s].p, nX * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int s = 0; s < 2; ++s) { const double v = -(ho[s] / (double)Ns); kls[s] = v > 0.0 ? v : 0.0; }   // vbmc_kldiv.m:77, :84, :88 (max ignores a NaN)
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_vp_mode(vbmc_ctx* ctx, const vbmc_vp_desc* vp, const vbmc_mode_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_mode";
  if (!args || args->struct_size != sizeof(vbmc_mode_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  if (!(args->tol_grad > 0.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: tol_grad must be positive", who);
  if (args->max_iter < 0 || args->max_iter > MODE_ITER_CAP) return set_err(ctx, VBMC_ERR_INVALID, "%s: max_iter = %d outside 0 .. %d", who, args->max_iter, MODE_ITER_CAP);
  if (!args->x || !args->fval || !args->idx) return set_err(ctx, VBMC_ERR_INVALID, "%s: x, fval and idx are required", who);
  VptPack pk;
  VB_TRY(vpt_pack(ctx, who, vp, 0.0, pk));
  return mode_run(ctx, vp, args, pk);
}

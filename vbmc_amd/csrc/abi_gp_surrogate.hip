// C-ABI entry points of the surrogate sampler: vbmc_gp_surrogate_sample and vbmc_gp_surrogate_sample_rng_dump (include/vbmc_hip.h).
// The kernels are gp_surrogate_kernels.h; the sampler is the ensemble slice sampler of is_core.h with this file's target: E ensembles
// decoupled from the hyper-samples, every candidate under all of them (k_gs_pred into Sg x E x C means and variances, k_gs_target
// into the E x C values), no limit on the records.  Host side: validation, the start (the caller's, or draws of k_vp_draw) clipped
// into the box and written into the sampler's walker buffer, the noise estimate (gp_pred.h: NnNoise) in the same stream in front of
// the chain, the closing k_gs_finish and the copies back.  The packing of a posterior and the split of a draw are vp_tools_host.h's.
#include "gp_surrogate_kernels.h"
#include "is_core.h"
#include "vp_tools_host.h"

#define GS_DEFAULT_NNN 20000
#define GS_MAX_E 64
#define GS_MAX_BYTES ((size_t)1 << 30)

extern "C" vbmc_status vbmc_gp_surrogate_sample_rng_dump(uint64_t seed, int E, int H, int M, double* U) {
  return vbmc_acq_is_sample_rng_dump(seed, E, H, M, U);
}

namespace {
// N unbalanced transformed-space draws of the posterior into X (N x D column-major, on the device): vbmc_vp_rnd(vp, N, 0, 0, seed)
vbmc_status gs_draw(vbmc_ctx* ctx, const char* who, const vbmc_vp_desc* vp, const VptPack& pk, long long N, unsigned long long seed, VptGenHost& g, double* X) {
  VB_TRY(vpt_gen_host(ctx, who, vp->K, vp->w, N, 0, seed, g));
  g.G.origflag = 0;
  VB_TRY(vpt_gen_upload(ctx, who, vp->D, nullptr, g));
  VptDrawArgs a{};
  a.P = pk.P; a.G = g.G; a.X = X; a.I = nullptr;
  const dim3 grid((unsigned)((N + VPT_T - 1) / VPT_T));
  VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_draw<DT>), grid, dim3(VPT_T), 0, ctx->stream, a))
  HIP_TRY(ctx, hipGetLastError());
  return VBMC_OK;
}
}  // namespace

extern "C" vbmc_status vbmc_gp_surrogate_sample(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_vp_desc* vp, const vbmc_gs_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_gp_surrogate_sample";
  if (!args || args->struct_size != sizeof(vbmc_gs_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const vbmc_gs_args& g = *args;
  if (!gp || !g.LB || !g.UB) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = gp->D, S = gp->S, N = gp->N, E = g.E;
  if (g.D != D || g.S != S)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the arrays are laid out for D = %d and S = %d, the GP has D = %d and S = %d hyper-samples", who, g.D, g.S, D, S);
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (g.rng_mode != 0 && g.rng_mode != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: rng_mode %d (0 device, 1 parity)", who, g.rng_mode);
  if (g.Ns < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld must be at least 1", who, (long long)g.Ns);
  if (E < 1 || E > GS_MAX_E) return set_err(ctx, VBMC_ERR_INVALID, "%s: E = %d outside 1 .. %d", who, E, GS_MAX_E);
  if (g.burnin < -1) return set_err(ctx, VBMC_ERR_INVALID, "%s: burnin must be non-negative (-1: ceil(Ns / 5))", who);
  if (g.beta != g.beta || std::isinf(g.beta)) return set_err(ctx, VBMC_ERR_INVALID, "%s: beta must be finite", who);
  const int W = g.W ? g.W : 2 * (D + 1);
  const long long nm_ll = (g.Ns + E - 1) / E;
  if ((double)nm_ll * E * D * 8.0 > (double)GS_MAX_BYTES)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: E Nm D = %d x %lld x %d doubles of records are more than 1 GiB", who, E, nm_ll, D);
  const int Nm = (int)nm_ll;
  const long long burn_ll = g.burnin >= 0 ? g.burnin : (g.Ns + 4) / 5;     // gplite_sample.m:71
  if (burn_ll > 0x3fffffff) return set_err(ctx, VBMC_ERR_INVALID, "%s: burnin = %lld is too large", who, burn_ll);
  const IsParams p{W, Nm, g.thin, (int)burn_ll, g.spec, g.max_steps, g.max_shrink, g.chunk, g.rng_mode, g.Mmax, g.seed, g.U};
  VB_TRY(is_check_params(ctx, who, D, E, 0, p));
  if ((long long)g.thin * Nm + burn_ll > 0x3fffffff) return set_err(ctx, VBMC_ERR_INVALID, "%s: burnin + thin Nm is too large", who);
  VB_TRY(check_box(ctx, who, g.LB, g.UB, 0, D));
  const bool noise = g.sn2new != nullptr;
  const int Nnn = g.Nnn ? g.Nnn : GS_DEFAULT_NNN;
  if (noise) {
    if (!g.X_rescaled || !g.gplengthscale) return set_err(ctx, VBMC_ERR_INVALID, "%s: the noise estimate needs X_rescaled and gplengthscale", who);
    if (Nnn < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nnn = %d", who, Nnn);
    for (int d = 0; d < D; ++d)
      if (!(std::isfinite(g.gplengthscale[d]) && g.gplengthscale[d] > 0.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: gplengthscale must be positive", who);
  }
  if (!vp && (!g.x0 || noise || g.origflag))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the variational posterior is needed (for the start without x0, the noise estimate and origflag)", who);
  VptPack pk;
  if (vp) {
    VB_TRY(vpt_pack(ctx, who, vp, 0.0, pk));
    if (vp->D != D) return set_err(ctx, VBMC_ERR_INVALID, "%s: the posterior has D = %d, the GP D = %d", who, vp->D, D);
  }
  const size_t n0 = (size_t)W * E * D;
  if (g.x0)
    for (size_t i = 0; i < n0; ++i)
      if (!std::isfinite(g.x0[i])) return set_err(ctx, VBMC_ERR_INVALID, "%s: a starting point is not finite", who);

  hipStream_t st = ctx->stream;
  const int nb = noise ? std::min((Nnn + GS_SUM_T - 1) / GS_SUM_T, VPT_MAXBLK) : 0;
  TmpBuf dV, dX0, dNn;
  NnNoise nn;
  const GsBlocks L(D, S, E, is_round_candidates(p), n0, noise ? Nnn : 0);
  HIP_TRY(ctx, dV.alloc(ctx, L.v.bytes()));
  double *d_vt = L.vt.at(dV.p), *d_sum = L.sum.at(dV.p), *d_part = L.part.at(dV.p);
  IsCore c;
  VB_TRY(is_core_begin(ctx, gp, who, p, E, L.extra, c));
  IsPredKernel pred;
  void (*gs_pred)(IsPredArgs) = nullptr;
  DISPATCH_QS(D, gs_pred = k_gs_pred<QS>)
  VB_TRY(pred.set(ctx, N, D, gs_pred));
  GsTargetArgs tg{};
  L.bind(tg, c.pg, c.d_extra, dV.p);
  tg.S = S; tg.E = E; tg.C = c.C; tg.nstride = c.pg.nstride; tg.ncand = c.pg.ncand; tg.mask = c.a.mask;
  tg.beta = g.beta; tg.val = c.d_val;
  std::vector<double> hb(c.L.UB.end() / 8), h0;            // the head of the sampler's block: LB | UB
  c.L.LB.put(hb.data(), g.LB); c.L.UB.put(hb.data(), g.UB);
  HIP_TRY(ctx, hipMemcpyAsync(c.dW.p, hb.data(), c.L.UB.end(), hipMemcpyHostToDevice, st));
  const double hvt[2] = {g.VarThresh, 0.0};
  HIP_TRY(ctx, hipMemcpyAsync(d_vt, hvt, sizeof hvt, hipMemcpyHostToDevice, st));
  if (vp) VB_TRY(vpt_upload(ctx, pk));

  // ---- the start: rows r = w + W e of a (W E) x D column-major buffer, clipped into the walker buffer and into x0_out's layout
  HIP_TRY(ctx, dX0.alloc(ctx, L.x0.bytes()));
  double *d_x0 = L.start.at(dX0.p), *d_x0c = L.clipped.at(dX0.p);
  VptGenHost gen0, genn;
  if (g.x0) {
    h0.resize(n0);
    const size_t n = (size_t)W * E;
    for (int e = 0; e < E; ++e)
      for (int d = 0; d < D; ++d)
        for (int w = 0; w < W; ++w) h0[(size_t)w + (size_t)W * e + n * d] = g.x0[w + (size_t)W * (d + (size_t)D * e)];
    HIP_TRY(ctx, hipMemcpyAsync(d_x0, h0.data(), n0 * 8, hipMemcpyHostToDevice, st));
  } else {
    VB_TRY(gs_draw(ctx, who, vp, pk, (long long)W * E, g.seed, gen0, d_x0));
  }
  hipLaunchKernelGGL(k_gs_start, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, W, D, E, d_x0, c.a.LB, c.a.UB, c.a.x, d_x0c);

  // ---- the noise estimate
  double* d_nn = nullptr;
  if (noise) {
    HIP_TRY(ctx, dNn.alloc(ctx, L.nn.bytes()));
    double* d_xx = L.draws.at(dNn.p);
    d_nn = L.sn2.at(dNn.p);
    VB_TRY(nn.upload(ctx, gp, g.gplengthscale, g.X_rescaled, g.sn2new));
    VB_TRY(gs_draw(ctx, who, vp, pk, Nnn, g.seed + 1, genn, d_xx));
    nn.launch(st, Nnn, d_xx, d_nn);
    hipLaunchKernelGGL(k_gs_sum, dim3(nb), dim3(GS_SUM_T), 0, st, Nnn, d_nn, d_part);
    hipLaunchKernelGGL(k_vp_reduce, dim3(1), dim3(VPT_T), 0, st, d_part, nb, 1, d_sum);
    hipLaunchKernelGGL(k_gs_thresh, dim3(1), dim3(64), 0, st, d_sum, Nnn, d_vt);
  }
  HIP_TRY(ctx, hipGetLastError());

  // ---- the chain: a round's candidates under every hyper-sample, then the target
  IsCounters n;
  const dim3 pgrid((c.C + 15) / 16, E, S), tgrid((c.C + 63) / 64, E);
  VB_TRY(is_core_run(ctx, who, p, c, [&] {
    pred.launch(st, pgrid, c.pg);
    hipLaunchKernelGGL(k_gs_target, tgrid, dim3(64), 0, st, tg);
  }, nullptr, n));
  is_write_counters(n, g.funccount, g.performed, g.rounds);

  // ---- the recorded walkers into X; the copies back
  const size_t nXo = (size_t)g.Ns * D, nr = (size_t)E * Nm;
  TmpBuf dXo;
  if (g.X) {
    HIP_TRY(ctx, dXo.alloc(ctx, nXo * 8));
    GsFinishArgs f{};
    if (g.origflag) f.P = pk.P;
    f.P.D = D;
    f.Ns = (int)g.Ns; f.Nm = Nm; f.E = E; f.origflag = g.origflag ? 1 : 0; f.Xa = c.a.Xa; f.X = dXo.as<double>();
    const dim3 grid((unsigned)((g.Ns + VPT_T - 1) / VPT_T));
    VPT_FOR_DT(vpt_pick_dt(D), hipLaunchKernelGGL((k_gs_finish<DT>), grid, dim3(VPT_T), 0, st, f))
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(g.X, f.X, nXo * 8, hipMemcpyDeviceToHost, st));
  }
  std::vector<double> hr;
  double hv[2] = {0.0, 0.0};
  if (g.Xt) HIP_TRY(ctx, hipMemcpyAsync(g.Xt, c.a.Xa, c.L.Xa.size(), hipMemcpyDeviceToHost, st));
  if (g.logp) { hr.resize(nr); HIP_TRY(ctx, hipMemcpyAsync(hr.data(), c.a.rlp, nr * 8, hipMemcpyDeviceToHost, st)); }
  if (g.x0_out) HIP_TRY(ctx, hipMemcpyAsync(g.x0_out, d_x0c, n0 * 8, hipMemcpyDeviceToHost, st));
  if (g.sn2_nn && noise) HIP_TRY(ctx, hipMemcpyAsync(g.sn2_nn, d_nn, (size_t)Nnn * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hv, d_vt, sizeof hv, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (g.logp) is_unpack_rows(hr, E, Nm, Nm, g.logp, 1, E);
  if (g.varthresh_out) *g.varthresh_out = hv[0];
  if (g.sn2_avg_out) *g.sn2_avg_out = hv[1];
  return VBMC_OK;
}

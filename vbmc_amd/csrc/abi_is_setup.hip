// C-ABI entry points of the one-call set-up of the IMIQR importance sampler: vbmc_acq_is_setup and vbmc_acq_is_setup_rng_dump
// (include/vbmc_hip.h).  Step 1 and the resampling are is_setup_kernels.h; the prediction of the Step 1 points is k_is_pred on the
// set-up the sampler uses anyway (every ensemble's point buffer holds the same Na1 points); the starting walkers are written where
// the sampler (is_core.h) expects them, so that Step 2 -- the IMIQR target of imiqr_target.h: imiqr_begin, imiqr_rounds,
// imiqr_close -- follows in the same stream.
#include "imiqr_target.h"
#include "is_core.h"
#include "is_setup_kernels.h"
#include "parity_rng.h"

extern "C" vbmc_status vbmc_acq_is_setup_rng_dump(uint64_t seed, int D, int S, int W, int Nvp, int Nbox, double* B) {
  if (D <= 0 || S <= 0 || W < 0 || Nvp < 0 || Nbox < 0 || Nvp + Nbox < 1 || !B) return VBMC_ERR_INVALID;
  const int Na1 = Nvp + Nbox;
  for (int i = 0; i < Na1; ++i) {
    B[(size_t)(D + 1) * i] = slice_uniform(seed, ISS_CTR_POINT, (unsigned)i, 0u);
    for (int d = 0; d < D; ++d)
      B[(size_t)(1 + d) + (size_t)(D + 1) * i] = i < Nvp ? srch_normal(seed, ISS_CTR_POINT, (unsigned)i, (unsigned)d) : slice_uniform(seed, ISS_CTR_POINT, (unsigned)i, (unsigned)(1 + d));
  }
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < W; ++i) B[(size_t)(D + 1) * Na1 + i + (size_t)W * s] = slice_uniform(seed, ISS_CTR_DRAW, (unsigned)s, (unsigned)i);
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_acq_is_setup(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_is_setup_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_acq_is_setup";
  if (args && args->struct_size == sizeof(vbmc_is_setup_args) && args->state) *args->state = nullptr;
  if (!args || args->struct_size != sizeof(vbmc_is_setup_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const vbmc_is_setup_args& g = *args;
  if (g.n_bad) *g.n_bad = 0;
  if (!gp || !g.vp_mu || !g.vp_sigma || !g.vp_lambda || !g.vp_w) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = gp->D, S = gp->S, N = gp->N, K = g.K, Nm = g.Nm;
  if (g.D != D || g.S != S)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the arrays are laid out for D = %d and S = %d, the GP has D = %d and S = %d hyper-samples", who, g.D, g.S, D, S);
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (K < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: K = %d", who, K);
  if (K > VBMC_LIM_K) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "K = %d > %d not accelerated", K, VBMC_LIM_K);
  if (g.Nvp < 0 || g.Nbox < 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nvp = %d and Nbox = %d must be non-negative", who, g.Nvp, g.Nbox);
  const long long na_ll = (long long)g.Nvp + g.Nbox;
  if (na_ll < 1 || na_ll > ISS_MAXNA) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nvp + Nbox = %lld outside 1 .. %d", who, na_ll, ISS_MAXNA);
  const int Na1 = (int)na_ll, Nap1 = ((Na1 + 15) / 16) * 16;
  if (N < 2) return set_err(ctx, VBMC_ERR_INVALID, "%s: rect_delta = 2 std(X) needs at least two training inputs", who);
  if (g.rng_mode != 0 && g.rng_mode != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: rng_mode %d (0 device, 1 parity)", who, g.rng_mode);
  if (Nm < 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nm = %d outside 0 .. %d", who, Nm, VBMC_LIM_NA);
  const bool step2 = Nm > 0;
  // Step 1 alone: the sampler's routines still provide the prediction's set-up, for the smallest sampler there is
  IsParams p{step2 ? g.W : 4, step2 ? Nm : 1, step2 ? g.thin : 1, step2 ? g.burnin : -1, g.spec, g.max_steps, g.max_shrink, g.chunk,
             (g.rng_mode == 1 && g.U && step2) ? 1 : 0, g.Mmax, g.seed, step2 ? g.U : nullptr};
  VB_TRY(is_check_params(ctx, who, D, S, VBMC_LIM_NA, p));
  const int W = step2 ? g.W : 0;
  double wsum = 0.0;
  bool vp_ok = true;
  for (int k = 0; k < K; ++k) {
    vp_ok = vp_ok && std::isfinite(g.vp_sigma[k]) && g.vp_sigma[k] > 0.0 && std::isfinite(g.vp_w[k]) && g.vp_w[k] >= 0.0;
    wsum += g.vp_w[k];
    for (int d = 0; d < D; ++d) vp_ok = vp_ok && std::isfinite(g.vp_mu[d + (size_t)D * k]);
  }
  for (int d = 0; d < D; ++d) vp_ok = vp_ok && std::isfinite(g.vp_lambda[d]) && g.vp_lambda[d] > 0.0;
  if (!vp_ok || !(wsum > 0.0) || !std::isfinite(wsum))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the variational posterior must be finite with sigma, lambda > 0 and weights >= 0 of positive sum", who);
  const size_t nB = g.rng_mode == 1 ? IsSetupBlock::block_len(D, S, W, Na1) : 0;
  if (g.rng_mode == 1) {
    if (!g.B) return set_err(ctx, VBMC_ERR_INVALID, "%s: parity mode needs the block B", who);
    for (size_t j = 0; j < nB; ++j) {
      const size_t i = j / (size_t)(D + 1), slot = j % (size_t)(D + 1);
      const bool normal = j < (size_t)(D + 1) * Na1 && (int)i < g.Nvp && slot > 0;
      const double v = g.B[j];
      if (normal ? !std::isfinite(v) : !(v > 0.0 && v < 1.0))
        return set_err(ctx, VBMC_ERR_INVALID, "%s: block value %zu: the uniforms must lie strictly inside (0, 1), the normals must be finite", who, j);
    }
  }

  IsCore c;
  ImiqrTarget t;
  VB_TRY(imiqr_begin(ctx, gp, who, p, c, t));
  hipStream_t st = ctx->stream;
  const IsSetupBlock L(D, S, K, W, Na1, g.rng_mode == 1);
  const size_t nX1 = L.Xa1.n, np1 = L.lnw1.n;
  TmpBuf d1, dIdx, dNc1;
  HIP_TRY(ctx, d1.alloc(ctx, L.L.bytes()));
  HIP_TRY(ctx, dIdx.alloc(ctx, (size_t)std::max(W, 1) * S * sizeof(int)));
  HIP_TRY(ctx, dNc1.alloc(ctx, (size_t)S * sizeof(int)));
  std::vector<double> hup(L.upload / 8);
  L.mu.put(hup.data(), g.vp_mu); L.sigma.put(hup.data(), g.vp_sigma); L.lambda.put(hup.data(), g.vp_lambda); L.w.put(hup.data(), g.vp_w);
  L.B.put(hup.data(), g.B);
  const std::vector<int> hnc1(S, Na1);
  HIP_TRY(ctx, hipMemcpyAsync(d1.p, hup.data(), L.upload, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dNc1.p, hnc1.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));

  IsSetupKArgs k{};
  k.D = D; k.N = N; k.S = S; k.K = K; k.Nvp = g.Nvp; k.Nbox = g.Nbox; k.W = W; k.parity = g.rng_mode; k.seed = g.seed;
  k.w_vp = (double)g.Nvp / (double)Na1;                // :110
  k.X = gp->X;
  L.bind(k, d1.p);
  k.LB = const_cast<double*>(c.a.LB); k.UB = const_cast<double*>(c.a.UB);
  k.x = c.a.x; k.idx0 = dIdx.as<int>();

  hipLaunchKernelGGL(k_is_draw, dim3(1), dim3(ISS_DRAW_THREADS), 0, st, k);
  IsPredArgs pg1 = c.pg;
  L.bind(pg1, d1.p);
  pg1.mask = nullptr; pg1.ncand = dNc1.as<int>(); pg1.nstride = 1; pg1.C = Na1;
  t.pk.launch(st, dim3((Na1 + 15) / 16, S), pg1);
  hipLaunchKernelGGL(k_is_proposal, dim3(Nap1), dim3(64), 0, st, k);
  if (step2) hipLaunchKernelGGL(k_is_resample, dim3(S), dim3(64), 0, st, k);
  HIP_TRY(ctx, hipGetLastError());

  // ---- Step 2 behind it in the same stream; the Step 1 arrays come back with whatever else the caller asked for
  IsBadStart bad;
  IsCounters n;
  if (step2) VB_TRY(imiqr_rounds(ctx, who, p, c, t, &bad, n));
  if (step2 && bad.n == 0) VB_TRY(imiqr_close(ctx, gp, who, c, t, n, {g.Xa, g.lnw, g.fs2a, g.logp, g.funccount, g.performed, g.rounds, g.state}));
  std::vector<double> hl, hf, hg;
  std::vector<int> hi;
  if (g.Xa1) HIP_TRY(ctx, hipMemcpyAsync(g.Xa1, k.Xa1, nX1 * 8, hipMemcpyDeviceToHost, st));
  if (g.lpdf1) HIP_TRY(ctx, hipMemcpyAsync(g.lpdf1, k.lpdf, (size_t)Na1 * 8, hipMemcpyDeviceToHost, st));
  if (g.lnw1) { hl.resize(np1); HIP_TRY(ctx, hipMemcpyAsync(hl.data(), k.lnw1, np1 * 8, hipMemcpyDeviceToHost, st)); }
  if (g.fs2a1) { hf.resize(np1); HIP_TRY(ctx, hipMemcpyAsync(hf.data(), k.fs2a1, np1 * 8, hipMemcpyDeviceToHost, st)); }
  if (g.rect_delta) HIP_TRY(ctx, hipMemcpyAsync(g.rect_delta, k.geo, (size_t)D * 8, hipMemcpyDeviceToHost, st));
  if (g.LB || g.UB) { hg.resize(2 * (size_t)D); HIP_TRY(ctx, hipMemcpyAsync(hg.data(), k.LB, 2 * (size_t)D * 8, hipMemcpyDeviceToHost, st)); }
  if (step2 && g.x0) HIP_TRY(ctx, hipMemcpyAsync(g.x0, k.x0, (size_t)W * D * S * 8, hipMemcpyDeviceToHost, st));
  if (step2 && g.idx0) { hi.resize((size_t)W * S); HIP_TRY(ctx, hipMemcpyAsync(hi.data(), k.idx0, (size_t)W * S * sizeof(int), hipMemcpyDeviceToHost, st)); }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (g.lnw1) is_unpack_rows(hl, S, Na1, Nap1, g.lnw1, 1, S);
  if (g.fs2a1) is_unpack_rows(hf, S, Na1, Nap1, g.fs2a1, Na1, 1);
  if (g.LB) memcpy(g.LB, hg.data(), (size_t)D * 8);
  if (g.UB) memcpy(g.UB, hg.data() + D, (size_t)D * 8);
  if (step2 && g.idx0) for (size_t j = 0; j < hi.size(); ++j) g.idx0[j] = hi[j];
  if (step2 && bad.n > 0) {
    if (g.n_bad) *g.n_bad = bad.n;
    if (g.bad) memcpy(g.bad, bad.mask.data(), (size_t)W * S);
    is_write_counters({(long long)W * S, (long long)W * S, 0, 0}, g.funccount, g.performed, g.rounds);
    return VBMC_OK;
  }
  if (step2 && g.bad) memset(g.bad, 0, (size_t)W * S);
  if (!step2) {
    is_write_counters({0, 0, 0, 0}, g.funccount, g.performed, g.rounds);
    // the state of the Na1 shared points with lnw1 (:148-157 with Nmcmc_samples = 0)
    if (g.state) VB_TRY(acq_is_from_device(ctx, gp, who, Na1, 0, k.Xa1, k.lnw1, k.fs2a1, g.state));
  }
  return VBMC_OK;
}

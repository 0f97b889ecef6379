// C-ABI entry points of the device-resident importance sampler: vbmc_acq_is_sample and vbmc_acq_is_sample_rng_dump
// (include/vbmc_hip.h): the ensemble slice sampler (is_core.h) on the IMIQR target (imiqr_target.h).
#include "imiqr_target.h"
#include "parity_rng.h"

extern "C" vbmc_status vbmc_acq_is_sample_rng_dump(uint64_t seed, int S, int H, int M, double* U) {
  if (S <= 0 || H <= 0 || M <= 0 || !U) return VBMC_ERR_INVALID;
  for (int m = 0; m < M; ++m)
    for (int e = 0; e < S; ++e)
      for (int j = 0; j < H; ++j)
        for (int k = 0; k < IS_SLOTS; ++k)
          U[(size_t)k + IS_SLOTS * ((size_t)j + (size_t)H * ((size_t)e + (size_t)S * m))] = slice_uniform(seed, (unsigned)m, (unsigned)(e * H + j), (unsigned)k);
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_acq_is_sample(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_is_sample_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_acq_is_sample";
  if (args && args->struct_size == sizeof(vbmc_is_sample_args) && args->state) *args->state = nullptr;
  if (!args || args->struct_size != sizeof(vbmc_is_sample_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const vbmc_is_sample_args& g = *args;
  if (!gp || !g.x0 || !g.LB || !g.UB) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  const int D = gp->D, S = gp->S, W = g.W;
  if (g.D != D || g.S != S)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: x0 is laid out as W x %d x %d, the GP has D = %d and S = %d hyper-samples", who, g.D, g.S, D, S);
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (g.rng_mode != 0 && g.rng_mode != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: rng_mode %d (0 device, 1 parity)", who, g.rng_mode);
  const IsParams p{g.W, g.Nm, g.thin, g.burnin, g.spec, g.max_steps, g.max_shrink, g.chunk, g.rng_mode, g.Mmax, g.seed, g.U};
  VB_TRY(is_check_params(ctx, who, D, S, VBMC_LIM_NA, p));
  VB_TRY(check_box(ctx, who, g.LB, g.UB, 0, D));
  for (int e = 0; e < S; ++e)
    for (int d = 0; d < D; ++d)
      for (int w = 0; w < W; ++w) {
        const double x = g.x0[w + (size_t)W * (d + (size_t)D * e)];
        if (!(x >= g.LB[d] && x <= g.UB[d]))
          return set_err(ctx, VBMC_ERR_INVALID, "%s: a starting point is outside the box (walker %d of ensemble %d, coordinate %d)", who, w + 1, e + 1, d + 1);
      }
  IsCore c;
  ImiqrTarget t;
  VB_TRY(imiqr_begin(ctx, gp, who, p, c, t));
  std::vector<double> hx(c.L.x.end() / 8);               // the head of the sampler's block: LB | UB | x
  c.L.LB.put(hx.data(), g.LB); c.L.UB.put(hx.data(), g.UB);
  double* hx0 = c.L.x.at(hx.data());
  for (int e = 0; e < S; ++e)
    for (int w = 0; w < W; ++w)
      for (int d = 0; d < D; ++d) hx0[((size_t)e * W + w) * D + d] = g.x0[w + (size_t)W * (d + (size_t)D * e)];
  HIP_TRY(ctx, hipMemcpyAsync(c.dW.p, hx.data(), c.L.x.end(), hipMemcpyHostToDevice, ctx->stream));
  IsCounters n;
  VB_TRY(imiqr_rounds(ctx, who, p, c, t, nullptr, n));
  return imiqr_close(ctx, gp, who, c, t, n, {g.Xa, g.lnw, g.fs2a, g.logp, g.funccount, g.performed, g.rounds, g.state});
}

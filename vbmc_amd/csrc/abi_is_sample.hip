// C-ABI entry points of the device-resident importance sampler: vbmc_acq_is_sample and vbmc_acq_is_sample_rng_dump
// (include/vbmc_hip.h), and the IMIQR target of the ensemble slice sampler (is_core.h) that vbmc_acq_is_setup (abi_is_setup.hip) runs
// too: one ensemble per hyper-sample, k_is_pred evaluating each ensemble's candidates under its own hyper-sample, at most VBMC_LIM_NA
// records.  imiqr_begin sets the sampler up with the target's buffers, imiqr_rounds runs it, imiqr_close is what follows the chain: one
// closing prediction at the recorded walkers, lnw and fs2a (k_is_finish), the outputs and the importance-sampling state
// (gp_pred.h: acq_is_from_device).
#include "is_core.h"

extern "C" vbmc_status vbmc_acq_is_sample_rng_dump(uint64_t seed, int S, int H, int M, double* U) {
  if (S <= 0 || H <= 0 || M <= 0 || !U) return VBMC_ERR_INVALID;
  for (int m = 0; m < M; ++m)
    for (int e = 0; e < S; ++e)
      for (int j = 0; j < H; ++j)
        for (int k = 0; k < IS_SLOTS; ++k)
          U[(size_t)k + IS_SLOTS * ((size_t)j + (size_t)H * ((size_t)e + (size_t)S * m))] = slice_uniform(seed, (unsigned)m, (unsigned)(e * H + j), (unsigned)k);
  return VBMC_OK;
}

namespace {
struct ImiqrOutputs {
  double *Xa, *lnw, *fs2a, *logp;
  int64_t *funccount, *performed, *rounds;
  vbmc_acq_is** state;
};
struct ImiqrTarget {
  IsPredKernel pk;              // k_is_pred<QS> for the GP's D
  TmpBuf dNc;
  std::vector<int> hnc;         // Nm per ensemble: the closing prediction's counts (alive until the stream has copied them)
  double *d_cl = nullptr, *d_lnw = nullptr, *d_fs2a = nullptr;
  size_t np = 0;
  int Nap = 0;
};

// behind the S x C values:  fmu fs2 ys2 (S x C each) | the closing prediction's logp fmu fs2 ys2 (S x Nm each) | lnw fs2a (S x Nap each)
vbmc_status imiqr_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, const IsParams& p, IsCore& c, ImiqrTarget& t) {
  const int S = gp->S, Nm = p.Nm;
  const size_t nv = (size_t)S * is_round_candidates(p), nr = (size_t)S * Nm;
  t.Nap = ((Nm + 15) / 16) * 16;
  t.np = (size_t)S * t.Nap;
  VB_TRY(is_core_begin(ctx, gp, who, p, S, 3 * nv + 4 * nr + 2 * t.np, c));
  HIP_TRY(ctx, t.dNc.alloc(ctx, (size_t)S * sizeof(int)));
  t.hnc.assign(S, Nm);
  HIP_TRY(ctx, hipMemcpyAsync(t.dNc.p, t.hnc.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  c.pg.fmu = c.d_extra; c.pg.fs2 = c.d_extra + nv; c.pg.ys2 = c.d_extra + 2 * nv;
  t.d_cl = c.d_extra + 3 * nv;
  t.d_lnw = t.d_cl + 4 * nr;
  t.d_fs2a = t.d_lnw + t.np;
  void (*f)(IsPredArgs) = nullptr;
  DISPATCH_QS(gp->D, f = k_is_pred<QS>)
  return t.pk.set(ctx, gp->N, gp->D, f);
}

// the chain: the prediction's workgroups of an ensemble whose step left no candidates return at once
vbmc_status imiqr_rounds(vbmc_ctx* ctx, const char* who, const IsParams& p, IsCore& c, const ImiqrTarget& t, IsBadStart* bad, IsCounters& n) {
  const dim3 grid((c.C + 15) / 16, c.a.S);
  return is_core_run(ctx, who, p, c, [&] { t.pk.launch(ctx->stream, grid, c.pg); }, bad, n);
}

vbmc_status imiqr_close(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, IsCore& c, ImiqrTarget& t, const IsCounters& n, const ImiqrOutputs& o) {
  hipStream_t st = ctx->stream;
  const IsStepArgs& a = c.a;
  const int S = a.S, Nm = a.Nm, Nap = t.Nap;
  const size_t nr = c.nr, np = t.np;
  // ---- one closing prediction at the recorded walkers (Xa is the point buffer of Nm slots per ensemble), lnw and fs2a
  IsPredArgs cg = c.pg;
  cg.P = a.Xa; cg.mask = nullptr; cg.ncand = t.dNc.as<int>(); cg.nstride = 1; cg.C = Nm;
  cg.logp = t.d_cl; cg.fmu = t.d_cl + nr; cg.fs2 = t.d_cl + 2 * nr; cg.ys2 = t.d_cl + 3 * nr;
  t.pk.launch(st, dim3((Nm + 15) / 16, S), cg);
  hipLaunchKernelGGL(k_is_finish, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, S, Nm, Nap, cg.fmu, cg.fs2, a.rlp, t.d_lnw, t.d_fs2a);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> hr, hl, hf;
  if (o.Xa) HIP_TRY(ctx, hipMemcpyAsync(o.Xa, a.Xa, c.nXa * 8, hipMemcpyDeviceToHost, st));
  if (o.logp) { hr.resize(nr); HIP_TRY(ctx, hipMemcpyAsync(hr.data(), a.rlp, nr * 8, hipMemcpyDeviceToHost, st)); }
  if (o.lnw) { hl.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hl.data(), t.d_lnw, np * 8, hipMemcpyDeviceToHost, st)); }
  if (o.fs2a) { hf.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hf.data(), t.d_fs2a, np * 8, hipMemcpyDeviceToHost, st)); }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (o.logp) is_unpack_rows(hr, S, Nm, Nm, o.logp, 1, S);
  if (o.lnw) is_unpack_rows(hl, S, Nm, Nap, o.lnw, 1, S);
  if (o.fs2a) is_unpack_rows(hf, S, Nm, Nap, o.fs2a, Nm, 1);
  is_write_counters(n, o.funccount, o.performed, o.rounds);
  if (o.state) VB_TRY(acq_is_from_device(ctx, gp, who, Nm, 1, a.Xa, t.d_lnw, t.d_fs2a, o.state));
  return VBMC_OK;
}
}  // namespace

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
  std::vector<double> hx(2 * (size_t)D + c.nx);
  memcpy(hx.data(), g.LB, (size_t)D * 8);
  memcpy(hx.data() + D, g.UB, (size_t)D * 8);
  for (int e = 0; e < S; ++e)
    for (int w = 0; w < W; ++w)
      for (int d = 0; d < D; ++d) hx[2 * (size_t)D + ((size_t)e * W + w) * D + d] = g.x0[w + (size_t)W * (d + (size_t)D * e)];
  HIP_TRY(ctx, hipMemcpyAsync(c.dW.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  IsCounters n;
  VB_TRY(imiqr_rounds(ctx, who, p, c, t, nullptr, n));
  return imiqr_close(ctx, gp, who, c, t, n, {g.Xa, g.lnw, g.fs2a, g.logp, g.funccount, g.performed, g.rounds, g.state});
}

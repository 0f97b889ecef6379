// The IMIQR target of the ensemble slice sampler (is_core.h), shared by vbmc_acq_is_sample (abi_is_sample.hip) and vbmc_acq_is_setup
// (abi_is_setup.hip): one ensemble per hyper-sample, k_is_pred evaluating each ensemble's candidates under its own hyper-sample, at most
// VBMC_LIM_NA records.  imiqr_begin sets the sampler up with the target's buffers, imiqr_rounds runs it, imiqr_close is what follows the
// chain: one closing prediction at the recorded walkers, lnw and fs2a (k_is_finish), the outputs and the importance-sampling state
// (gp_pred.h: acq_is_from_device).
#pragma once
#include <vector>

#include "is_core.h"

namespace {
struct ImiqrOutputs {
  double *Xa, *lnw, *fs2a, *logp;
  int64_t *funccount, *performed, *rounds;
  vbmc_acq_is** state;
};
// The target's region behind the sampler's S x C values (is_core.h), from the shape alone; Nap: Nm rounded up to whole tiles of 16
//   fmu fs2 ys2 (S x C each) | the closing prediction's logp fmu fs2 ys2 (S x Nm each) | lnw fs2a (S x Nap each)
struct ImiqrExtra {
  DevLayout L;
  int Nap = 0;
  DevWin<double> fmu, fs2, ys2, cl_logp, cl_fmu, cl_fs2, cl_ys2, lnw, fs2a;
  ImiqrExtra() {}
  ImiqrExtra(int S, int C, int Nm) : Nap(((Nm + 15) / 16) * 16) {
    const size_t nv = (size_t)S * C, nr = (size_t)S * Nm, np = (size_t)S * Nap;
    fmu = L.add<double>(nv); fs2 = L.add<double>(nv); ys2 = L.add<double>(nv);
    cl_logp = L.add<double>(nr); cl_fmu = L.add<double>(nr); cl_fs2 = L.add<double>(nr); cl_ys2 = L.add<double>(nr);
    lnw = L.add<double>(np); fs2a = L.add<double>(np);
  }
  void bind(IsPredArgs& g, void* base) const { g.fmu = fmu.at(base); g.fs2 = fs2.at(base); g.ys2 = ys2.at(base); }                // a round's
  void bind_closing(IsPredArgs& g, void* base) const { g.logp = cl_logp.at(base); g.fmu = cl_fmu.at(base); g.fs2 = cl_fs2.at(base); g.ys2 = cl_ys2.at(base); }
};
struct ImiqrTarget {
  IsPredKernel pk;              // k_is_pred<QS> for the GP's D
  TmpBuf dNc;
  std::vector<int> hnc;         // Nm per ensemble: the closing prediction's counts (alive until the stream has copied them)
  ImiqrExtra x;                 // its region behind the sampler's values; the windows resolve against IsCore::d_extra
};

vbmc_status imiqr_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, const IsParams& p, IsCore& c, ImiqrTarget& t) {
  const int S = gp->S, Nm = p.Nm;
  t.x = ImiqrExtra(S, is_round_candidates(p), Nm);
  VB_TRY(is_core_begin(ctx, gp, who, p, S, t.x.L, c));
  HIP_TRY(ctx, t.dNc.alloc(ctx, (size_t)S * sizeof(int)));
  t.hnc.assign(S, Nm);
  HIP_TRY(ctx, hipMemcpyAsync(t.dNc.p, t.hnc.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  t.x.bind(c.pg, c.d_extra);
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
  const int S = a.S, Nm = a.Nm, Nap = t.x.Nap;
  const size_t nr = c.L.rlp.n, np = t.x.lnw.n;
  double *d_lnw = t.x.lnw.at(c.d_extra), *d_fs2a = t.x.fs2a.at(c.d_extra);
  // ---- one closing prediction at the recorded walkers (Xa is the point buffer of Nm slots per ensemble), lnw and fs2a
  IsPredArgs cg = c.pg;
  cg.P = a.Xa; cg.mask = nullptr; cg.ncand = t.dNc.as<int>(); cg.nstride = 1; cg.C = Nm;
  t.x.bind_closing(cg, c.d_extra);
  t.pk.launch(st, dim3((Nm + 15) / 16, S), cg);
  hipLaunchKernelGGL(k_is_finish, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, S, Nm, Nap, cg.fmu, cg.fs2, a.rlp, d_lnw, d_fs2a);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> hr, hl, hf;
  if (o.Xa) HIP_TRY(ctx, hipMemcpyAsync(o.Xa, a.Xa, c.L.Xa.size(), hipMemcpyDeviceToHost, st));
  if (o.logp) { hr.resize(nr); HIP_TRY(ctx, hipMemcpyAsync(hr.data(), a.rlp, nr * 8, hipMemcpyDeviceToHost, st)); }
  if (o.lnw) { hl.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hl.data(), d_lnw, np * 8, hipMemcpyDeviceToHost, st)); }
  if (o.fs2a) { hf.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hf.data(), d_fs2a, np * 8, hipMemcpyDeviceToHost, st)); }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (o.logp) is_unpack_rows(hr, S, Nm, Nm, o.logp, 1, S);
  if (o.lnw) is_unpack_rows(hl, S, Nm, Nap, o.lnw, 1, S);
  if (o.fs2a) is_unpack_rows(hf, S, Nm, Nap, o.fs2a, Nm, 1);
  is_write_counters(n, o.funccount, o.performed, o.rounds);
  if (o.state) VB_TRY(acq_is_from_device(ctx, gp, who, Nm, 1, a.Xa, d_lnw, d_fs2a, o.state));
  return VBMC_OK;
}
}  // namespace

// Host side of the ensemble slice sampler (is_sample_kernels.h: k_is_step), shared by the entry points that sample with it and
// knowing none of their targets.  A target brings: the number of ensembles E, a limit on the records per ensemble if it has one, the
// doubles it wants behind the E x C values k_is_step reads, a kernel of k_is_pred's shape picked for the GP's D (IsPredKernel), and a
// callable that enqueues the evaluation of a round's candidates into those values.  The core owns the parameters and their checks,
// the prediction's per-hyper-sample set-up (k_pred_prep of gp_pred.h's pred_plan, centred on the training inputs alone), the state
// block, the uniforms, the rounds (drive_rounds of round_driver.h, the E progress words read one chunk behind the one being
// enqueued) under their cap, the ensembles' final states with their errors, and the report of starts of zero density.  It returns the
// run's counters and leaves the recorded walkers c.a.Xa and their values c.a.rlp on the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "gp_pred.h"
#include "is_sample_kernels.h"
#include "round_driver.h"

#define IS_DEFAULT_CHUNK 16
#define IS_DEFAULT_SPEC 3

namespace {
// the sampler's parameters as the entry points take them, defaults still unresolved
struct IsParams {
  int W, Nm, thin, burnin, spec, max_steps, max_shrink, chunk, parity, Mmax;
  unsigned long long seed;
  const double* U;              // parity: IS_SLOTS x H x E x Mmax (host)
};
inline int is_round_candidates(const IsParams& g) { return 2 * (g.spec ? g.spec : IS_DEFAULT_SPEC) * (g.W / 2); }   // C: at the most (>= W)
struct IsCounters { long long funccount = 0, performed = 0, rounds = 0, behind = 0; };
struct IsBadStart {             // is_core_run with one: a start of zero density is reported here instead of being an error
  int n = 0;
  std::vector<unsigned char> mask;   // W x E
};
// a kernel of k_is_pred's shape: its owner picks the instantiation for the GP's D; the dynamic LDS of its tile is allowed once per call
// where it needs more than the default 64 KB
struct IsPredKernel {
  void (*fn)(IsPredArgs) = nullptr;
  size_t lds = 0;
  vbmc_status set(vbmc_ctx* ctx, int N, int D, void (*f)(IsPredArgs)) {
    if (!f) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", D);
    fn = f;
    lds = ISP_LDS_BYTES(((N + 15) >> 4) << 4);
    if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return VBMC_OK;
  }
  void launch(hipStream_t st, dim3 grid, const IsPredArgs& g) const { hipLaunchKernelGGL(fn, grid, dim3(ISP_THREADS), lds, st, g); }
};
struct IsCore {
  PredBufs pb;
  PredPlan pl;
  TmpBuf dW, dSt, dWk, dMask;
  IsStepArgs a{};
  IsPredArgs pg{};              // the set-up, the point buffer, its mask and counts, logp = the values; the outputs are the target's
  IsCoreBlock L;                // dW's layout
  double* d_val = nullptr;      // E x C values
  void* d_extra = nullptr;      // the base of the target's region behind them
  int C = 0;
};

inline void is_write_counters(const IsCounters& n, int64_t* funccount, int64_t* performed, int64_t* rounds) {
  if (funccount) *funccount = n.funccount;
  if (performed) *performed = n.performed;
  if (rounds) { rounds[0] = n.rounds; rounds[1] = n.behind; }
}
// rows of ld values on the host, the first n of each: dst[ds s + di i] = src[ld s + i]
inline void is_unpack_rows(const std::vector<double>& src, int S, int n, size_t ld, double* dst, size_t ds, size_t di) {
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < n; ++i) dst[ds * s + di * i] = src[ld * s + i];
}

// nm_limit: the most records per ensemble the target can take (0: no limit)
vbmc_status is_check_params(vbmc_ctx* ctx, const char* who, int D, int E, int nm_limit, const IsParams& g) {
  const int W = g.W, H = W / 2, Nm = g.Nm;
  if (W < 4 || W % 2 != 0 || W > 2 * (D + 1)) return set_err(ctx, VBMC_ERR_INVALID, "%s: W = %d must be even with 4 <= W <= 2 (D + 1) = %d", who, W, 2 * (D + 1));
  if (Nm < 1 || (nm_limit && Nm > nm_limit)) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nm = %d outside 1 .. %d", who, Nm, VBMC_LIM_NA);
  if (g.thin < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: thin must be at least 1", who);
  if (g.burnin < -1) return set_err(ctx, VBMC_ERR_INVALID, "%s: burnin must be non-negative (-1: ceil(thin Nm / 2))", who);
  if (g.spec < 0 || g.spec > IS_MAXSPEC) return set_err(ctx, VBMC_ERR_INVALID, "%s: spec = %d outside 1 .. %d (0: %d)", who, g.spec, IS_MAXSPEC, IS_DEFAULT_SPEC);
  if (g.max_steps < 0 || g.max_steps > IS_MAXSTEPS || g.max_shrink < 0 || g.max_shrink > IS_MAXSHRINK)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: max_steps / max_shrink outside 1 .. %d / 1 .. %d (0: the caps)", who, IS_MAXSTEPS, IS_MAXSHRINK);
  if (g.chunk < 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: chunk must be non-negative", who);
  if (g.parity && (!g.U || g.Mmax < 1)) return set_err(ctx, VBMC_ERR_INVALID, "%s: parity mode needs U and Mmax >= 1", who);
  if (g.parity) {
    const size_t nu = (size_t)IS_SLOTS * H * E * g.Mmax;
    for (size_t i = 0; i < nu; ++i)
      if (!(g.U[i] > 0.0 && g.U[i] < 1.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: the uniforms must lie strictly inside (0, 1)", who);
  }
  return VBMC_OK;
}

// The prediction's per-hyper-sample set-up, the sampler's device state (zeroed, the target's region with it) and its uniforms.
// What is left to the caller before is_core_run: the outputs of c.pg and the kernel for it, the box c.a.LB / c.a.UB and the E x W x D
// starting walkers c.a.x, on the device, in the context's stream.
vbmc_status is_core_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, const IsParams& g, int E, const DevLayout& target, IsCore& c) {
  VB_TRY(pred_check(ctx, who, gp, 16, false));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = gp->N, D = gp->D, W = g.W, H = W / 2, Nm = g.Nm;
  PredBufs& pb = c.pb;
  PredPlan& pl = c.pl;
  // the per-hyper-sample set-up of the prediction (dXc, daa, dmuv; inv(L') on the GP handle), centred on the training inputs alone
  HIP_TRY(ctx, pb.dXs.alloc(ctx, (size_t)16 * D * 8));
  HIP_TRY(ctx, pb.dmb.alloc(ctx, (size_t)D * 8));
  VB_TRY(pred_plan(ctx, gp, 16, pb, false, nullptr, pl));
  if (pl.f.slab_pred)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: N = %d is beyond the range in which the prediction keeps inv(L') resident", who, N);
  pl.pa.mc = 0;
  HIP_TRY(ctx, hipMemsetAsync(pb.dmb.p, 0, (size_t)D * 8, st));
  hipLaunchKernelGGL(k_pred_prep, dim3(4, gp->S), dim3(256), 0, st, pl.pa, pb.dXc.as<double>(), pb.daa.as<double>(), pb.dmuv.as<double>());

  IsStepArgs& a = c.a;
  a.D = D; a.S = E; a.W = W; a.H = H; a.Nm = Nm; a.thin = g.thin;
  a.burnin = g.burnin >= 0 ? g.burnin : (int)(((long long)g.thin * Nm + 1) / 2);
  a.spec = g.spec ? g.spec : IS_DEFAULT_SPEC;
  a.max_steps = g.max_steps ? g.max_steps : IS_MAXSTEPS;
  a.max_shrink = g.max_shrink ? g.max_shrink : IS_MAXSHRINK;
  a.parity = g.parity; a.Mmax = g.Mmax; a.seed = g.seed;
  const int C = is_round_candidates(g);
  a.C = C;
  c.C = C;
  const size_t nU = g.parity ? (size_t)IS_SLOTS * H * E * g.Mmax : 0, nv = (size_t)E * C;
  c.L = IsCoreBlock(D, E, W, C, Nm, target, nU);
  const IsCoreBlock& L = c.L;
  HIP_TRY(ctx, c.dW.alloc(ctx, L.w.bytes()));
  HIP_TRY(ctx, c.dSt.alloc(ctx, (size_t)E * sizeof(IsEnsState)));
  HIP_TRY(ctx, c.dWk.alloc(ctx, (size_t)E * IS_MAXH * sizeof(IsWalker)));
  HIP_TRY(ctx, c.dMask.alloc(ctx, nv));
  VB_TRY(ensure_pin(ctx, 2 * (size_t)E * sizeof(IsEnsState) + 64));       // two landing slots of the progress words
  HIP_TRY(ctx, hipMemsetAsync(c.dW.p, 0, L.fixed, st));
  HIP_TRY(ctx, hipMemsetAsync(c.dSt.p, 0, (size_t)E * sizeof(IsEnsState), st));
  HIP_TRY(ctx, hipMemsetAsync(c.dWk.p, 0, (size_t)E * IS_MAXH * sizeof(IsWalker), st));
  HIP_TRY(ctx, hipMemsetAsync(c.dMask.p, 0, nv, st));
  L.bind(a, c.dW.p);
  c.d_val = L.val.at(c.dW.p);
  c.d_extra = L.extra.at(c.dW.p);
  a.st = c.dSt.as<IsEnsState>(); a.wk = c.dWk.as<IsWalker>(); a.mask = c.dMask.as<unsigned char>();
  if (nU) HIP_TRY(ctx, hipMemcpyAsync(L.U.at(c.dW.p), g.U, L.U.size(), hipMemcpyHostToDevice, st));

  IsPredArgs& pg = c.pg;
  pg.pa = pl.pa;
  pg.Xc = pb.dXc.as<double>(); pg.aa = pb.daa.as<double>(); pg.muv = pb.dmuv.as<double>();
  pg.P = a.P; pg.mask = a.mask; pg.ncand = &a.st->ncand; pg.nstride = (int)(sizeof(IsEnsState) / sizeof(int)); pg.C = C;
  pg.logp = c.d_val;
  return VBMC_OK;
}

// The rounds from the starting walkers on the device to Nm recorded walkers per ensemble.  A round is the sampler's step, then eval():
// the target at the candidates the step wrote.  A step that finds its chain finished does nothing and leaves no candidates.
// (a chain needs at most max_steps + max_shrink + 1 rounds per half-move and two to start; the read-behind adds chunks of idle rounds:
// a count beyond that means the progress words never reported the end, and the call stops instead of enqueueing for ever)
template <class Eval>
vbmc_status is_core_run(vbmc_ctx* ctx, const char* who, const IsParams& g, IsCore& c, Eval eval, IsBadStart* bad, IsCounters& out) {
  hipStream_t st = ctx->stream;
  IsStepArgs& a = c.a;
  const int E = a.S, W = a.W, H = a.H, Nm = a.Nm, C = c.C;
  const int chunk = g.chunk > 0 ? g.chunk : IS_DEFAULT_CHUNK;
  const long long halfmoves = ((long long)a.burnin + (long long)Nm * a.thin + H - 1) / H;
  const long long round_cap = halfmoves * (a.max_steps + a.max_shrink + 1) + 2 + 4 * (long long)chunk + 8;
  long long enqueued = 0;
  auto round = [&](int) -> vbmc_status {
    if (++enqueued > round_cap) return set_err(ctx, VBMC_ERR_HIP, "%s: the chain did not finish within %lld rounds", who, round_cap);
    hipLaunchKernelGGL(k_is_step, dim3(E), dim3(64), 0, st, a);
    eval();
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  };
  VB_TRY(drive_rounds(ctx, who, chunk, round, c.dSt.p, (size_t)E * sizeof(IsEnsState), (size_t)E * sizeof(IsEnsState), [E, bad](const char* p) {
    const IsEnsState* s = (const IsEnsState*)p;
    for (int e = 0; e < E; ++e)
      if (bad && s[e].err == IS_ERR_START) return Progress::finished;     // the caller gets the starts back: nothing more to enqueue
    for (int e = 0; e < E; ++e)
      if (!s[e].done) return Progress::running;
    return Progress::finished;
  }, chunk));
  std::vector<IsEnsState> fin(E);
  HIP_TRY(ctx, hipMemcpy(fin.data(), c.dSt.p, (size_t)E * sizeof(IsEnsState), hipMemcpyDeviceToHost));
  if (bad) {                                           // the starts of an ensemble that stopped there still have their values in place
    std::vector<double> hv;
    bad->mask.assign((size_t)W * E, 0);
    for (int e = 0; e < E; ++e) {
      if (fin[e].err != IS_ERR_START) continue;
      hv.resize(W);
      HIP_TRY(ctx, hipMemcpy(hv.data(), c.d_val + (size_t)e * C, (size_t)W * 8, hipMemcpyDeviceToHost));
      for (int w = 0; w < W; ++w)
        if (!std::isfinite(hv[w])) { bad->mask[w + (size_t)W * e] = 1; bad->n += 1; }
    }
    if (bad->n > 0) return VBMC_OK;
  }
  out = IsCounters{0, 0, 0, -1};
  for (int e = 0; e < E; ++e) {
    if (fin[e].err == IS_ERR_START) return set_err(ctx, VBMC_ERR_INVALID, "%s: a starting point has zero density (ensemble %d)", who, e + 1);
    if (fin[e].err == IS_ERR_UNIFORMS)
      return set_err(ctx, VBMC_ERR_INVALID, "%s: uniform block exhausted: the chain needed more than Mmax = %d half-moves", who, g.Mmax);
    if (!fin[e].done) return set_err(ctx, VBMC_ERR_HIP, "%s: the chain did not finish", who);
    out.funccount += fin[e].funccount; out.performed += fin[e].performed;
    out.rounds = std::max<long long>(out.rounds, fin[e].rounds);
    out.behind = out.behind < 0 ? fin[e].behind : std::min<long long>(out.behind, fin[e].behind);
  }
  return VBMC_OK;
}
}  // namespace

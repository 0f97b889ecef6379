// C-ABI entry points of the device-resident importance sampler: vbmc_acq_is_sample and vbmc_acq_is_sample_rng_dump
// (include/vbmc_hip.h), and the routines it shares with vbmc_acq_is_setup (abi_is_setup.hip): is_core_begin, is_core_run.  The sampler is is_sample_kernels.h: k_is_step writes a round's candidates into the point buffer, k_is_pred
// evaluates each under its own hyper-sample on the per-hyper-sample set-up of k_pred_prep (abi_gp.hip: pred_plan, run once per call with
// the centring constant of the training inputs alone).  Rounds are driven in chunks by drive_rounds (abi_gp_train.hip), the S progress
// words read one chunk behind the one being enqueued.  The importance-sampling state is made of the device buffers where they are
// (abi_gp.hip: acq_is_new, acq_is_ctmp_resident).  The same two routines run the surrogate sampler (abi_gp_surrogate.hip) by a target
// kind in IsParams: E ensembles decoupled from the hyper-samples, k_gs_pred and k_gs_target in the round, no limit on Nm, no closing
// prediction.  Included after abi_acq_search.hip.
#include <algorithm>
#include <cmath>

#include "gp_surrogate_kernels.h"   // is_sample_kernels.h, and the surrogate sampler's kernels (abi_gp_surrogate.hip)

#define IS_DEFAULT_CHUNK 16
#define IS_DEFAULT_SPEC 3

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
// k_is_pred<QS> for the GP's D: the kernel, and its dynamic LDS allowed once per call where the tile needs more than the default 64 KB
struct IsPredKernel {
  void (*fn)(IsPredArgs) = nullptr;
  size_t lds = 0;
  vbmc_status pick(vbmc_ctx* ctx, int N, int D, bool surrogate = false) {
    const int Np = ((N + 15) >> 4) << 4;
    lds = ISP_LDS_BYTES(Np);
    switch ((D + 3) / 4) {
#define ISP_CASE(QSV) case QSV: fn = surrogate ? k_gs_pred<QSV> : k_is_pred<QSV>; break;
      ISP_CASE(1) ISP_CASE(2) ISP_CASE(3) ISP_CASE(4) ISP_CASE(5) ISP_CASE(6) ISP_CASE(7) ISP_CASE(8)
#undef ISP_CASE
      default: return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", D);
    }
    if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return VBMC_OK;
  }
  void launch(hipStream_t st, const IsPredArgs& g, int ntile) const { hipLaunchKernelGGL(fn, dim3(ntile, g.pa.S), dim3(ISP_THREADS), lds, st, g); }
  void launch_surrogate(hipStream_t st, const IsPredArgs& g, int ntile, int E) const { hipLaunchKernelGGL(fn, dim3(ntile, E, g.pa.S), dim3(ISP_THREADS), lds, st, g); }
};

// What vbmc_acq_is_sample and vbmc_acq_is_setup share: the sampler's parameters with their defaults still unresolved, and the outputs
struct IsParams {
  int W, Nm, thin, burnin, spec, max_steps, max_shrink, chunk, parity, Mmax;
  unsigned long long seed;
  const double* U;              // parity: IS_SLOTS x H x S x Mmax (host)
  // the target: IS_TARGET_IMIQR -- one ensemble per hyper-sample, each under its own, at most VBMC_LIM_NA records, the closing
  // prediction and the importance weights; IS_TARGET_SURROGATE -- E ensembles, every candidate under all hyper-samples (k_gs_pred,
  // k_gs_target), Nm unbounded, no closing (abi_gp_surrogate.hip finishes)
  int target = 0, E = 0;
  double beta = 0.0;
  const double* d_vt = nullptr; // IS_TARGET_SURROGATE: VarThresh on the device
};
enum { IS_TARGET_IMIQR = 0, IS_TARGET_SURROGATE = 1 };
inline int is_ensembles(const vbmc_gp* gp, const IsParams& g) { return g.target == IS_TARGET_SURROGATE ? g.E : gp->S; }
struct IsOutputs {
  double *Xa, *lnw, *fs2a, *logp;
  int64_t *funccount, *performed, *rounds;
  vbmc_acq_is** state;
};
struct IsBadStart {             // is_core_run with one: a start of zero density is reported here instead of being an error
  int n = 0;
  std::vector<unsigned char> mask;   // W x S
};
struct IsCore {
  PredBufs pb;
  PredPlan pl;
  TmpBuf dW, dSt, dWk, dMask, dNc;
  IsStepArgs a{};
  IsPredArgs pg{};
  IsPredKernel pk;
  GsTargetArgs tg{};            // IS_TARGET_SURROGATE
  double *d_val = nullptr, *d_cl = nullptr, *d_lnw = nullptr, *d_fs2a = nullptr;
  size_t nx = 0, nv = 0, nXa = 0, nr = 0, np = 0;
  int C = 0, Nap = 0;
  std::vector<int> hnc;         // Nm per ensemble: the closing prediction's counts (alive until the stream has copied them)
};

vbmc_status is_check_params(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, const IsParams& g) {
  const int D = gp->D, S = is_ensembles(gp, g), W = g.W, H = W / 2, Nm = g.Nm;
  if (W < 4 || W % 2 != 0 || W > 2 * (D + 1)) return set_err(ctx, VBMC_ERR_INVALID, "%s: W = %d must be even with 4 <= W <= 2 (D + 1) = %d", who, W, 2 * (D + 1));
  if (Nm < 1 || (g.target == IS_TARGET_IMIQR && Nm > VBMC_LIM_NA)) return set_err(ctx, VBMC_ERR_INVALID, "%s: Nm = %d outside 1 .. %d", who, Nm, VBMC_LIM_NA);
  if (g.thin < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: thin must be at least 1", who);
  if (g.burnin < -1) return set_err(ctx, VBMC_ERR_INVALID, "%s: burnin must be non-negative (-1: ceil(thin Nm / 2))", who);
  if (g.spec < 0 || g.spec > IS_MAXSPEC) return set_err(ctx, VBMC_ERR_INVALID, "%s: spec = %d outside 1 .. %d (0: %d)", who, g.spec, IS_MAXSPEC, IS_DEFAULT_SPEC);
  if (g.max_steps < 0 || g.max_steps > IS_MAXSTEPS || g.max_shrink < 0 || g.max_shrink > IS_MAXSHRINK)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: max_steps / max_shrink outside 1 .. %d / 1 .. %d (0: the caps)", who, IS_MAXSTEPS, IS_MAXSHRINK);
  if (g.chunk < 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: chunk must be non-negative", who);
  if (g.parity && (!g.U || g.Mmax < 1)) return set_err(ctx, VBMC_ERR_INVALID, "%s: parity mode needs U and Mmax >= 1", who);
  if (g.parity) {
    const size_t nu = (size_t)IS_SLOTS * H * S * g.Mmax;
    for (size_t i = 0; i < nu; ++i)
      if (!(g.U[i] > 0.0 && g.U[i] < 1.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: the uniforms must lie strictly inside (0, 1)", who);
  }
  return VBMC_OK;
}

// The prediction's per-hyper-sample set-up, the sampler's device state (zeroed) and its uniforms.  What is left to the caller before
// is_core_run: the box c.a.LB / c.a.UB and the S x W x D starting walkers c.a.x, on the device, in the context's stream.
vbmc_status is_core_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, const IsParams& g, IsCore& c) {
  VB_TRY(pred_check(ctx, who, gp, 16, false));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool surr = g.target == IS_TARGET_SURROGATE;
  const int N = gp->N, D = gp->D, Sg = gp->S, S = is_ensembles(gp, g), W = g.W, H = W / 2, Nm = g.Nm;   // S: the ensembles
  PredBufs& pb = c.pb;
  PredPlan& pl = c.pl;
  // the per-hyper-sample set-up of the prediction (dXc, daa, dmuv; inv(L') on the GP handle), centred on the training inputs alone
  HIP_TRY(ctx, pb.dXs.alloc(ctx, (size_t)16 * D * 8));
  HIP_TRY(ctx, pb.dmb.alloc(ctx, (size_t)D * 8));
  VB_TRY(pred_plan(ctx, gp, 16, pb, false, nullptr, pl));
  if (pl.slab_pred)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: N = %d is beyond the range in which the prediction keeps inv(L') resident", who, N);
  pl.pa.mc = 0;
  HIP_TRY(ctx, hipMemsetAsync(pb.dmb.p, 0, (size_t)D * 8, st));
  hipLaunchKernelGGL(k_pred_prep, dim3(4, Sg), dim3(256), 0, st, pl.pa, pb.dXc.as<double>(), pb.daa.as<double>(), pb.dmuv.as<double>());

  IsStepArgs& a = c.a;
  a.D = D; a.S = S; a.W = W; a.H = H; a.Nm = Nm; a.thin = g.thin;
  a.burnin = g.burnin >= 0 ? g.burnin : (int)(((long long)g.thin * Nm + 1) / 2);
  a.spec = g.spec ? g.spec : IS_DEFAULT_SPEC;
  a.max_steps = g.max_steps ? g.max_steps : IS_MAXSTEPS;
  a.max_shrink = g.max_shrink ? g.max_shrink : IS_MAXSHRINK;
  a.parity = g.parity; a.Mmax = g.Mmax; a.seed = g.seed;
  const int C = 2 * a.spec * H;                        // candidates of a round at the most (>= W)
  a.C = C;
  c.C = C;
  const int Nap = ((Nm + 15) / 16) * 16;
  c.Nap = Nap;
  // one block of fp64 state:  LB | UB | x | lp | P | val fmu fs2 ys2 | Xa | rlp | closing fmu fs2 | lnw fs2a (S x Nap) | U
  // (the surrogate's target:  ... | val  ymu ys2 (Sg x E x C each) | Xa | rlp | U)
  const size_t nU = g.parity ? (size_t)IS_SLOTS * H * S * g.Mmax : 0;
  const size_t nx = (size_t)S * W * D, nP = (size_t)S * D * C, nv = (size_t)S * C, nXa = (size_t)Nm * D * S, nr = (size_t)S * Nm, np = surr ? 0 : (size_t)S * Nap;
  const size_t nval = surr ? nv + 2 * (size_t)Sg * nv : 4 * nv, ncl = surr ? 0 : 4 * nr;
  const size_t n_fixed = 2 * (size_t)D + nx + (size_t)S * W + nP + nval + nXa + nr + ncl + 2 * np;
  c.nx = nx; c.nv = nv; c.nXa = nXa; c.nr = nr; c.np = np;
  HIP_TRY(ctx, c.dW.alloc(ctx, (n_fixed + nU) * 8));
  HIP_TRY(ctx, c.dSt.alloc(ctx, (size_t)S * sizeof(IsEnsState)));
  HIP_TRY(ctx, c.dWk.alloc(ctx, (size_t)S * IS_MAXH * sizeof(IsWalker)));
  HIP_TRY(ctx, c.dMask.alloc(ctx, nv));
  HIP_TRY(ctx, c.dNc.alloc(ctx, (size_t)S * sizeof(int)));
  VB_TRY(ensure_pin(ctx, 2 * (size_t)S * sizeof(IsEnsState) + 64));       // two landing slots of the progress words
  HIP_TRY(ctx, hipMemsetAsync(c.dW.p, 0, n_fixed * 8, st));
  HIP_TRY(ctx, hipMemsetAsync(c.dSt.p, 0, (size_t)S * sizeof(IsEnsState), st));
  HIP_TRY(ctx, hipMemsetAsync(c.dWk.p, 0, (size_t)S * IS_MAXH * sizeof(IsWalker), st));
  HIP_TRY(ctx, hipMemsetAsync(c.dMask.p, 0, nv, st));
  double* q = c.dW.as<double>();
  a.LB = q; q += D;
  a.UB = q; q += D;
  a.x = q; q += nx;
  a.lp = q; q += (size_t)S * W;
  a.P = q; q += nP;
  c.d_val = q; q += nval;
  a.val = c.d_val;
  a.Xa = q; q += nXa;
  a.rlp = q; q += nr;
  c.d_cl = q; q += ncl;                                // closing prediction: logp | fmu | fs2 | ys2, S x Nm each
  c.d_lnw = q; q += np;
  c.d_fs2a = q; q += np;
  a.U = nU ? q : nullptr;
  a.st = c.dSt.as<IsEnsState>(); a.wk = c.dWk.as<IsWalker>(); a.mask = c.dMask.as<unsigned char>();
  if (nU) HIP_TRY(ctx, hipMemcpyAsync(c.dW.as<double>() + n_fixed, g.U, nU * 8, hipMemcpyHostToDevice, st));
  c.hnc.assign(S, Nm);
  HIP_TRY(ctx, hipMemcpyAsync(c.dNc.p, c.hnc.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));

  IsPredArgs& pg = c.pg;
  pg.pa = pl.pa;
  pg.Xc = pb.dXc.as<double>(); pg.aa = pb.daa.as<double>(); pg.muv = pb.dmuv.as<double>();
  pg.P = a.P; pg.mask = a.mask; pg.ncand = &a.st->ncand; pg.nstride = (int)(sizeof(IsEnsState) / sizeof(int)); pg.C = C;
  pg.logp = c.d_val; pg.fmu = c.d_val + nv; pg.fs2 = c.d_val + 2 * nv; pg.ys2 = c.d_val + 3 * nv;
  if (surr) {                                          // ymu | ys2, Sg x E x C each, behind the E x C values
    pg.fs2 = nullptr; pg.ys2 = c.d_val + nv + (size_t)Sg * nv;
    GsTargetArgs& tg = c.tg;
    tg.S = Sg; tg.E = S; tg.C = C; tg.nstride = pg.nstride; tg.ncand = pg.ncand; tg.mask = a.mask; tg.ymu = pg.fmu; tg.ys2 = pg.ys2;
    tg.vt = g.d_vt; tg.beta = g.beta; tg.val = c.d_val;
  }
  VB_TRY(c.pk.pick(ctx, N, D, surr));
  return VBMC_OK;
}

// The rounds from the starting walkers on the device to Nm recorded walkers per ensemble, the closing prediction, lnw, fs2a, the
// outputs and the importance-sampling state.
vbmc_status is_core_run(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, const IsParams& g, IsCore& c, const IsOutputs& o, IsBadStart* bad) {
  hipStream_t st = ctx->stream;
  IsStepArgs& a = c.a;
  IsPredArgs& pg = c.pg;
  IsPredKernel& pk = c.pk;
  const bool surr = g.target == IS_TARGET_SURROGATE;
  const int S = a.S, W = a.W, H = a.H, Nm = a.Nm, C = c.C, Nap = c.Nap;   // S: the ensembles
  const size_t nv = c.nv, nXa = c.nXa, nr = c.nr, np = c.np;
  double *d_cl = c.d_cl, *d_lnw = c.d_lnw, *d_fs2a = c.d_fs2a;
  TmpBuf& dSt = c.dSt;
  const int ntile = (C + 15) / 16;
  // a round: the sampler's step, then the prediction and the target at the candidates it wrote.  A step that finds its chain finished
  // does nothing and leaves no candidates: the prediction's workgroups of that ensemble return at once.
  // (a chain needs at most max_steps + max_shrink + 1 rounds per half-move and two to start; the read-behind adds chunks of idle rounds:
  // a count beyond that means the progress words never reported the end, and the call stops instead of enqueueing for ever)
  const long long halfmoves = ((long long)a.burnin + (long long)Nm * a.thin + H - 1) / H;
  const long long round_cap = halfmoves * (a.max_steps + a.max_shrink + 1) + 2 + 4 * (long long)(g.chunk > 0 ? g.chunk : IS_DEFAULT_CHUNK) + 8;
  long long enqueued = 0;
  auto round = [&](int) -> vbmc_status {
    if (++enqueued > round_cap) return set_err(ctx, VBMC_ERR_HIP, "%s: the chain did not finish within %lld rounds", who, round_cap);
    hipLaunchKernelGGL(k_is_step, dim3(S), dim3(64), 0, st, a);
    if (surr) {
      pk.launch_surrogate(st, pg, ntile, S);
      hipLaunchKernelGGL(k_gs_target, dim3((C + 63) / 64, S), dim3(64), 0, st, c.tg);
    } else {
      pk.launch(st, pg, ntile);
    }
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  };
  const int chunk = g.chunk > 0 ? g.chunk : IS_DEFAULT_CHUNK;
  VB_TRY(drive_rounds(ctx, who, chunk, round, dSt.p, (size_t)S * sizeof(IsEnsState), (size_t)S * sizeof(IsEnsState), [S, bad](const char* p) {
    const IsEnsState* s = (const IsEnsState*)p;
    for (int e = 0; e < S; ++e)
      if (bad && s[e].err == IS_ERR_START) return Progress::finished;     // the caller gets the starts back: nothing more to enqueue
    for (int e = 0; e < S; ++e)
      if (!s[e].done) return Progress::running;
    return Progress::finished;
  }, chunk));
  std::vector<IsEnsState> fin(S);
  HIP_TRY(ctx, hipMemcpy(fin.data(), dSt.p, (size_t)S * sizeof(IsEnsState), hipMemcpyDeviceToHost));
  if (bad) {                                           // the starts of an ensemble that stopped there still have their values in place
    std::vector<double> hv;
    bad->mask.assign((size_t)W * S, 0);
    for (int e = 0; e < S; ++e) {
      if (fin[e].err != IS_ERR_START) continue;
      hv.resize(W);
      HIP_TRY(ctx, hipMemcpy(hv.data(), c.d_val + (size_t)e * C, (size_t)W * 8, hipMemcpyDeviceToHost));
      for (int w = 0; w < W; ++w)
        if (!std::isfinite(hv[w])) { bad->mask[w + (size_t)W * e] = 1; bad->n += 1; }
    }
    if (bad->n > 0) return VBMC_OK;
  }
  long long funccount = 0, performed = 0, rounds = 0, behind = -1;
  for (int e = 0; e < S; ++e) {
    if (fin[e].err == IS_ERR_START) return set_err(ctx, VBMC_ERR_INVALID, "%s: a starting point has zero density (ensemble %d)", who, e + 1);
    if (fin[e].err == IS_ERR_UNIFORMS)
      return set_err(ctx, VBMC_ERR_INVALID, "%s: uniform block exhausted: the chain needed more than Mmax = %d half-moves", who, g.Mmax);
    if (!fin[e].done) return set_err(ctx, VBMC_ERR_HIP, "%s: the chain did not finish", who);
    funccount += fin[e].funccount; performed += fin[e].performed;
    rounds = std::max<long long>(rounds, fin[e].rounds);
    behind = behind < 0 ? fin[e].behind : std::min<long long>(behind, fin[e].behind);
  }
  if (surr) {                                          // the recorded walkers stay on the device: the caller finishes
    if (o.funccount) *o.funccount = funccount;
    if (o.performed) *o.performed = performed;
    if (o.rounds) { o.rounds[0] = rounds; o.rounds[1] = behind; }
    return VBMC_OK;
  }
  // ---- one closing prediction at the recorded walkers (Xa is the point buffer of Nm slots per ensemble), lnw and fs2a
  IsPredArgs cg = pg;
  cg.P = a.Xa; cg.mask = nullptr; cg.ncand = c.dNc.as<int>(); cg.nstride = 1; cg.C = Nm;
  cg.logp = d_cl; cg.fmu = d_cl + nr; cg.fs2 = d_cl + 2 * nr; cg.ys2 = d_cl + 3 * nr;
  pk.launch(st, cg, (Nm + 15) / 16);
  hipLaunchKernelGGL(k_is_finish, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, S, Nm, Nap, cg.fmu, cg.fs2, a.rlp, d_lnw, d_fs2a);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> hr, hl, hf;
  if (o.Xa) HIP_TRY(ctx, hipMemcpyAsync(o.Xa, a.Xa, nXa * 8, hipMemcpyDeviceToHost, st));
  if (o.logp) { hr.resize(nr); HIP_TRY(ctx, hipMemcpyAsync(hr.data(), a.rlp, nr * 8, hipMemcpyDeviceToHost, st)); }
  if (o.lnw) { hl.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hl.data(), d_lnw, np * 8, hipMemcpyDeviceToHost, st)); }
  if (o.fs2a) { hf.resize(np); HIP_TRY(ctx, hipMemcpyAsync(hf.data(), d_fs2a, np * 8, hipMemcpyDeviceToHost, st)); }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < Nm; ++i) {
      if (o.logp) o.logp[s + (size_t)S * i] = hr[(size_t)s * Nm + i];
      if (o.lnw) o.lnw[s + (size_t)S * i] = hl[(size_t)s * Nap + i];
      if (o.fs2a) o.fs2a[i + (size_t)Nm * s] = hf[(size_t)s * Nap + i];
    }
  if (o.funccount) *o.funccount = funccount;
  if (o.performed) *o.performed = performed;
  if (o.rounds) { o.rounds[0] = rounds; o.rounds[1] = behind; }
  if (o.state) {
    vbmc_acq_is* h = nullptr;
    VB_TRY(acq_is_new(ctx, gp, Nm, 1, true, &h));
    auto fail = [&](vbmc_status s_) { vbmc_acq_is_free(ctx, h); return s_; };
    hipError_t e1 = hipMemcpyAsync(h->Xa, a.Xa, nXa * 8, hipMemcpyDeviceToDevice, st);
    hipError_t e2 = hipMemcpyAsync(h->lnw, d_lnw, np * 8, hipMemcpyDeviceToDevice, st);
    hipError_t e3 = hipMemcpyAsync(h->fs2a, d_fs2a, np * 8, hipMemcpyDeviceToDevice, st);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(set_err(ctx, VBMC_ERR_HIP, "%s: device copy into the state failed", who));
    const vbmc_status cs = acq_is_ctmp_resident(ctx, gp, h);
    if (cs != VBMC_OK) return fail(cs);
    *o.state = h;
  }
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
  VB_TRY(is_check_params(ctx, who, gp, p));
  for (int d = 0; d < D; ++d) {
    const double lb = g.LB[d], ub = g.UB[d];
    if (!std::isfinite(lb) || !std::isfinite(ub) || !(lb < ub))
      return set_err(ctx, VBMC_ERR_INVALID, "%s: the box needs finite bounds with LB < UB (coordinate %d: [%g, %g])", who, d + 1, lb, ub);
  }
  for (int e = 0; e < S; ++e)
    for (int d = 0; d < D; ++d)
      for (int w = 0; w < W; ++w) {
        const double x = g.x0[w + (size_t)W * (d + (size_t)D * e)];
        if (!(x >= g.LB[d] && x <= g.UB[d]))
          return set_err(ctx, VBMC_ERR_INVALID, "%s: a starting point is outside the box (walker %d of ensemble %d, coordinate %d)", who, w + 1, e + 1, d + 1);
      }
  IsCore c;
  VB_TRY(is_core_begin(ctx, gp, who, p, c));
  std::vector<double> hx(2 * (size_t)D + c.nx);
  memcpy(hx.data(), g.LB, (size_t)D * 8);
  memcpy(hx.data() + D, g.UB, (size_t)D * 8);
  for (int e = 0; e < S; ++e)
    for (int w = 0; w < W; ++w)
      for (int d = 0; d < D; ++d) hx[2 * (size_t)D + ((size_t)e * W + w) * D + d] = g.x0[w + (size_t)W * (d + (size_t)D * e)];
  HIP_TRY(ctx, hipMemcpyAsync(c.dW.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  const IsOutputs o{g.Xa, g.lnw, g.fs2a, g.logp, g.funccount, g.performed, g.rounds, g.state};
  return is_core_run(ctx, gp, who, p, c, o, nullptr);
}

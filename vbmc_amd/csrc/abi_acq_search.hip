// C-ABI entry points of the device-resident acquisition search: vbmc_acq_search, vbmc_acq_search_iqr and vbmc_acq_search_rng_dump
// (include/vbmc_hip.h).  The optimiser is search_kernels.h; the objective is the prediction (gp_pred.h: pred_plan once, pred_launch
// per generation, on points and column means the optimiser's kernel writes into the prediction's own buffers) followed by k_acq
// (AcqConsts: the density-based functions) or by the tile form of the IQR functions (IqrTileObjective, iqr_tile_kernels.h).  Both entry
// points are search_impl; generations are driven in chunks by drive_rounds (round_driver.h), the progress word read one chunk behind
// the one being enqueued.
#include <algorithm>
#include <cmath>

#include "gp_pred.h"
#include "iqr_tile_kernels.h"
#include "parity_rng.h"
#include "round_driver.h"
#include "search_kernels.h"

#define SEARCH_DEFAULT_CHUNK 16

extern "C" vbmc_status vbmc_acq_search_rng_dump(uint64_t seed, int D, int lam, int G, double* Z) {
  if (D <= 0 || lam <= 0 || G <= 0 || !Z) return VBMC_ERR_INVALID;
  for (int g = 0; g < G; ++g)
    for (int j = 0; j < lam; ++j)
      for (int d = 0; d < D; ++d) Z[d + (size_t)D * (j + (size_t)lam * g)] = srch_normal(seed, (unsigned)g, (unsigned)j, (unsigned)d);
  return VBMC_OK;
}

namespace {
// What the IQR objective reads besides the prediction and the importance-sampling state: the inputs of the nearest-neighbour noise,
// uploaded once per search.  launch() enqueues k_nn_noise, the tile kernel and the closing kernel on the points a.Xs holds.
struct IqrTileObjective {
  NnNoise nn;
  TmpBuf dsx, drec, dacqs;
  IqrTileArgs a{};
  int NT = 1, W = 1;
  vbmc_status upload(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acq_is* is, int lam, const vbmc_acqsearch_args& g) {
    const int N = gp->N, D = gp->D, S = gp->S;
    NT = is->Nap / 16;
    W = std::max(1, std::min(IQRT_MAXW, (N + 15) / 16));
    VB_TRY(nn.upload(ctx, gp, g.gplengthscale, g.X_rescaled, g.sn2new));
    HIP_TRY(ctx, dsx.alloc(ctx, (size_t)lam * 8));
    HIP_TRY(ctx, drec.alloc(ctx, (size_t)S * NT * 32 * 8));
    HIP_TRY(ctx, dacqs.alloc(ctx, (size_t)lam * S * 8));
    a = IqrTileArgs{};
    a.N = N; a.D = D; a.S = S; a.Nhyp = gp->Nhyp; a.lam = lam; a.Na = is->Na; a.Nap = is->Nap; a.per_s = is->per_s;
    a.reg = g.var_regularized ? 1 : 0; a.TolVar = g.TolGPVar;
    a.Xa = is->Xa; a.hyp = gp->hyp; a.CT = is->CT; a.fs2a = is->fs2a; a.lnw = is->has_lnw ? is->lnw : nullptr;
    a.sn2_eff = gp->d_sn2; a.lchol = gp->d_lchol; a.sn2x = dsx.as<double>(); a.rec = drec.as<double>(); a.acqs = dacqs.as<double>();
    return VBMC_OK;
  }
  void launch(hipStream_t st) {
    nn.launch(st, a.lam, a.Xs, dsx.as<double>());      // lam <= SRCH_MAXLAM = 16 points: one workgroup
    hipLaunchKernelGGL(k_acq_iqr_tile, dim3(NT, a.S), dim3(64 * W), IQRT_LDS_BYTES(W), st, a);
    hipLaunchKernelGGL(k_iqr_tile_final, dim3(1), dim3(64), 0, st, a, NT);
  }
};

// is == nullptr: the density-based functions (vbmc_acq_search); otherwise the IQR functions on that state (vbmc_acq_search_iqr)
vbmc_status search_impl(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, const vbmc_acq_is* is, bool iqr, const vbmc_acqsearch_args* args) {
  if (!args || args->struct_size != sizeof(vbmc_acqsearch_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const vbmc_acqsearch_args& g = *args;
  if (!gp || !g.x0 || !g.insigma || !g.LB || !g.UB) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  if (iqr) {
    if (!is) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
    if (g.acq_id != 10 && g.acq_id != 11)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: acquisition function id %d is not an IQR function (10 acqviqr, 11 acqimiqr)", who, g.acq_id);
    if (!g.gplengthscale || !g.X_rescaled || !g.sn2new)
      return set_err(ctx, VBMC_ERR_INVALID, "%s: the IQR functions need gplengthscale, X_rescaled and sn2new", who);
    if (is->N != gp->N || is->S != gp->S || is->D != gp->D)
      return set_err(ctx, VBMC_ERR_INVALID, "%s: importance-sampling state belongs to a different GP", who);
  } else {
    if (g.K <= 0 || !g.vp_mu || !g.vp_sigma || !g.vp_lambda || !g.vp_w) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
    if (g.acq_id >= 10) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: the importance-sampled IQR acquisition functions (id %d) are not searched on the device", who, g.acq_id);
    if (g.acq_id < 0 || g.acq_id > 3)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "acquisition function id %d not accelerated (0 acqf, 1 acqflog, 2 acqus, 3 acqfsn2)", g.acq_id);
    if (g.acq_id == 3 && (!g.gplengthscale || !g.X_rescaled || !g.sn2new))
      return set_err(ctx, VBMC_ERR_INVALID, "%s: acqfsn2 needs gplengthscale, X_rescaled and sn2new", who);
  }
  const int D = gp->D;
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (g.vp_delta)
    for (int d = 0; d < D; ++d)
      if (g.vp_delta[d] != 0.0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: vp.delta > 0 (gplite_quad, acqwrapper_vbmc.m:12-14) is not searched on the device", who);
  if (g.popsize != 0 && (g.popsize < 2 || g.popsize > SRCH_MAXLAM))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: popsize = %d outside 2 .. %d (0: 4 + floor(3 ln D))", who, g.popsize, SRCH_MAXLAM);
  const int lam = g.popsize ? g.popsize : 4 + (int)std::floor(3.0 * std::log((double)D));
  if (lam > SRCH_MAXLAM) return set_err(ctx, VBMC_ERR_INVALID, "%s: popsize = %d outside 2 .. %d", who, lam, SRCH_MAXLAM);
  double sigma0 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double lb = g.LB[d], ub = g.UB[d], x = g.x0[d], s = g.insigma[d];
    VB_TRY(check_box(ctx, who, g.LB, g.UB, d, d + 1));
    if (!(x >= lb && x <= ub)) return set_err(ctx, VBMC_ERR_INVALID, "%s: the start x0 is outside the box (coordinate %d: %g not in [%g, %g])", who, d + 1, x, lb, ub);
    if (!(s > 0.0) || !std::isfinite(s)) return set_err(ctx, VBMC_ERR_INVALID, "%s: insigma must be positive and finite", who);
    sigma0 = std::max(sigma0, s);
  }
  if (!(g.TolX >= 0.0) || !(g.TolFun >= 0.0) || !(g.TolHistFun >= 0.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: the tolerances must be non-negative", who);
  if (g.MaxIter < 0 || g.chunk < 0 || g.trace_cap < 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: MaxIter, chunk and trace_cap must be non-negative", who);
  if (g.rng_mode != 0 && g.rng_mode != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: rng_mode %d (0 device, 1 parity)", who, g.rng_mode);
  if (g.rng_mode == 1 && (!g.Z || g.Gmax < 1)) return set_err(ctx, VBMC_ERR_INVALID, "%s: parity mode needs Z and Gmax >= 1", who);
  const bool trace = g.tr_order || g.tr_F || g.tr_xmean || g.tr_sigma;
  if (trace && !(g.tr_order && g.tr_F && g.tr_xmean && g.tr_sigma && g.trace_cap > 0))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the trace needs tr_order, tr_F, tr_xmean, tr_sigma and trace_cap > 0", who);
  VB_TRY(pred_check(ctx, who, gp, lam, false));
  if (iqr && (is->Nap < 16 || is->Nap > VBMC_LIM_NA || is->Nap % 16)) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Na = %d not accelerated", is->Na);

  // ---- the constants of cmaes_batched (vbmc_amd/optimize.py), in its order of operations
  const int mu = lam / 2;
  std::vector<double> wts(mu);
  double wsum = 0.0, w2 = 0.0;
  for (int k = 0; k < mu; ++k) { wts[k] = std::log(mu + 0.5) - std::log((double)(k + 1)); wsum += wts[k]; }
  for (int k = 0; k < mu; ++k) { wts[k] /= wsum; w2 += wts[k] * wts[k]; }
  const double Nd = D, mueff = 1.0 / w2;
  SearchArgs a{};
  a.D = D; a.lam = lam; a.mu = mu; a.nh = 10 + (int)std::ceil(30.0 * Nd / lam);
  a.mueff = mueff;
  a.cc = (4 + mueff / Nd) / (Nd + 4 + 2 * mueff / Nd);
  a.cs = (mueff + 2) / (Nd + mueff + 5);
  a.c1 = 2 / ((Nd + 1.3) * (Nd + 1.3) + mueff);
  a.cmu = std::min(1 - a.c1, 2 * (mueff - 2 + 1 / mueff) / ((Nd + 2) * (Nd + 2) + mueff));
  a.damps = 1 + 2 * std::max(0.0, std::sqrt((mueff - 1) / (Nd + 1)) - 1) + a.cs;
  a.chiN = std::sqrt(Nd) * (1 - 1 / (4 * Nd) + 1 / (21 * Nd * Nd));
  a.tolx = g.TolX; a.tolfun = g.TolFun; a.tolhistfun = g.TolHistFun;
  a.max_evals = g.MaxFunEvals;
  a.max_iter = g.MaxIter > 0 ? g.MaxIter : (int)std::min(1e9, 1e3 * (Nd + 5) * (Nd + 5) / std::sqrt((double)lam));
  a.parity = g.rng_mode; a.Gmax = g.Gmax; a.seed = g.seed; a.trace_cap = trace ? g.trace_cap : 0;

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PredBufs pb;
  PredPlan pl;
  AcqConsts ac;
  IqrTileObjective iq;
  HIP_TRY(ctx, pb.dXs.alloc(ctx, (size_t)lam * D * 8));
  HIP_TRY(ctx, pb.dmb.alloc(ctx, (size_t)D * 8));
  // the IQR form keeps the sW-scaled cross-kernel tile (want_ks) and centres sq_dist on the training inputs alone (PredArgs::mc)
  VB_TRY(pred_plan(ctx, gp, lam, pb, iqr, nullptr, pl));
  if (iqr) {
    pl.pa.mc = 0;
    VB_TRY(iq.upload(ctx, gp, is, lam, g));
  } else {
    const AcqInputs in{g.acq_id, g.K, g.vp_mu, g.vp_sigma, g.vp_lambda, g.vp_w, g.ymax, g.var_regularized, g.TolGPVar, g.gplengthscale, g.X_rescaled, g.sn2new};
    VB_TRY(ac.upload(ctx, who, gp, lam, in));
  }
  const size_t nZ = g.rng_mode == 1 ? (size_t)D * lam * g.Gmax : 0;
  const size_t tcap = a.trace_cap;
  const SearchBlocks L(D, lam, mu, a.nh, nZ, tcap);                       // one block of fp64 state, one of the trace's
  TmpBuf dW, dState, dTrI, dTrD;
  HIP_TRY(ctx, dW.alloc(ctx, L.w.bytes()));
  HIP_TRY(ctx, dState.alloc(ctx, sizeof(SearchState)));
  if (tcap) {
    HIP_TRY(ctx, dTrI.alloc(ctx, tcap * lam * sizeof(int)));
    HIP_TRY(ctx, dTrD.alloc(ctx, L.trd.bytes()));
    HIP_TRY(ctx, hipMemsetAsync(dTrI.p, 0, tcap * lam * sizeof(int), st));
    HIP_TRY(ctx, hipMemsetAsync(dTrD.p, 0, L.trd.bytes(), st));
  }
  VB_TRY(ensure_pin(ctx, 2 * sizeof(SearchState) + 64));                  // two landing slots of the progress word
  std::vector<double> hw(L.fixed / 8, 0.0);
  L.wts.put(hw.data(), wts.data()); L.LB.put(hw.data(), g.LB); L.UB.put(hw.data(), g.UB);
  L.xmean.put(hw.data(), g.x0); L.xbest.put(hw.data(), g.x0); L.xlast.put(hw.data(), g.x0);
  for (int d = 0; d < D; ++d) { const double sc = g.insigma[d] / sigma0; L.C.at(hw.data())[d + (size_t)D * d] = sc * sc; }   // the initial C: diagonal
  L.bind(a, dW.p, dTrD.p);
  ac.a.acq = iq.a.acq = L.F.at(dW.p); ac.a.fbar = iq.a.fbar = L.fbar.at(dW.p); ac.a.vtot = iq.a.vtot = L.vtot.at(dW.p);
  HIP_TRY(ctx, hipMemcpyAsync(dW.p, hw.data(), L.fixed, hipMemcpyHostToDevice, st));
  if (nZ) HIP_TRY(ctx, hipMemcpyAsync(L.Z.at(dW.p), g.Z, L.Z.size(), hipMemcpyHostToDevice, st));
  SearchState s0{};
  s0.sigma = sigma0; s0.fbest = INFINITY; s0.flast = INFINITY;
  HIP_TRY(ctx, hipMemcpyAsync(dState.p, &s0, sizeof(SearchState), hipMemcpyHostToDevice, st));
  a.st = dState.as<SearchState>();
  a.Xs = pb.dXs.as<double>(); a.mb = pb.dmb.as<double>();
  ac.a.Xs = pb.dXs.as<double>(); ac.a.fmu = pb.fmu; ac.a.fs2 = pb.fs2;
  iq.a.Xs = pb.dXs.as<double>(); iq.a.fmu = pb.fmu; iq.a.fs2 = pb.fs2; iq.a.muv = pb.dmuv.as<double>(); iq.a.KsW = pb.dKs.as<double>();
  if (tcap) a.tr_order = dTrI.as<int>();
  // a generation: the optimiser's step, then the objective at the points it wrote.  A step that finds the search finished does
  // nothing; the prediction and the acquisition kernels behind it still run on the last points (their results are never read).
  auto round = [&](int) -> vbmc_status {
    hipLaunchKernelGGL(k_search_step, dim3(1), dim3(64), 0, st, a);
    VB_TRY(pred_launch(ctx, pb, pl));
    if (iqr) iq.launch(st);
    else ac.launch(st);
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  };
  const int chunk = g.chunk > 0 ? g.chunk : SEARCH_DEFAULT_CHUNK;
  VB_TRY(drive_rounds(ctx, who, chunk, round, dState.p, sizeof(SearchState), sizeof(SearchState), [](const char* p) {
    return ((const SearchState*)p)->done ? Progress::finished : Progress::running;
  }, chunk));
  SearchState fin;
  HIP_TRY(ctx, hipMemcpy(&fin, dState.p, sizeof(SearchState), hipMemcpyDeviceToHost));
  if (fin.err == SRCH_ERR_NORMALS)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: normal block exhausted: the search needed more than Gmax = %d generations", who, g.Gmax);
  if (!fin.done) return set_err(ctx, VBMC_ERR_HIP, "%s: the search did not finish", who);
  if (g.xmin) HIP_TRY(ctx, hipMemcpy(g.xmin, a.xlast, (size_t)D * 8, hipMemcpyDeviceToHost));
  if (g.xbest) HIP_TRY(ctx, hipMemcpy(g.xbest, a.xbest, (size_t)D * 8, hipMemcpyDeviceToHost));
  if (g.xmean) HIP_TRY(ctx, hipMemcpy(g.xmean, a.xmean, (size_t)D * 8, hipMemcpyDeviceToHost));
  if (g.C) HIP_TRY(ctx, hipMemcpy(g.C, a.C, (size_t)D * D * 8, hipMemcpyDeviceToHost));
  if (tcap) {
    HIP_TRY(ctx, hipMemcpy(g.tr_order, a.tr_order, tcap * lam * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(g.tr_F, a.tr_F, tcap * lam * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(g.tr_xmean, a.tr_xmean, tcap * D * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(g.tr_sigma, a.tr_sigma, tcap * 8, hipMemcpyDeviceToHost));
  }
  if (g.fmin) *g.fmin = fin.flast;
  if (g.fbest) *g.fbest = fin.fbest;
  if (g.sigma) *g.sigma = fin.sigma;
  if (g.evals) *g.evals = fin.evals;
  if (g.generations) *g.generations = fin.gen;
  if (g.stop) *g.stop = fin.stop;
  if (g.rounds) { g.rounds[0] = fin.gen; g.rounds[1] = fin.behind; }
  return VBMC_OK;
}
}  // namespace

extern "C" vbmc_status vbmc_acq_search(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acqsearch_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  return search_impl(ctx, "vbmc_acq_search", gp, nullptr, false, args);
}

extern "C" vbmc_status vbmc_acq_search_iqr(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acq_is* is, const vbmc_acqsearch_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  return search_impl(ctx, "vbmc_acq_search_iqr", gp, is, true, args);
}

// Device-resident acquisition search (private/activesample_vbmc.m:264-290 with SearchOptimizer = 'cmaes'): the plain
// (mu/mu_w, lambda)-CMA-ES of vbmc_amd/optimize.py::cmaes_batched in its Cholesky form (Krause, Arnold & Glasmachers 2016) inside a
// box, the optimiser's state on the device.  One GENERATION is
//   k_search_step   consume the previous generation's lambda acquisition values (rank, update xmean / ps / pc / C / sigma, the bests,
//                   the history ring, the stopping rules, the progress word), factorise C, draw or read Z, write the lambda clamped
//                   points and their column means straight into the prediction's device buffers
//   the prediction of <= 16 points x S hyper-samples (gp_pred.h: pred_launch) and k_acq, which leave the lambda values on the device.
// One workgroup of one wave: D <= 32, lambda <= 16.  The optimiser's own arithmetic is written with plain operators in scopes with
// contraction off and every sum runs in index order, so that a trajectory is a function of (Z, F) alone -- not of the chunking, not of
// the launch that happens to run it.
#pragma once
#include "common.h"
#include "dev_layout.h"
#include "parity_rng.h"

#define SRCH_MAXD 32
#define SRCH_MAXLAM 16
static_assert(SRCH_MAXD >= VBMC_LIM_D, "k_search_step keeps D x D matrices in LDS arrays of SRCH_MAXD");
enum { SRCH_STOP_NONE = 0, SRCH_STOP_TOLX = 1, SRCH_STOP_TOLFUN = 2, SRCH_STOP_TOLHISTFUN = 3, SRCH_STOP_MAXFUNEVALS = 4, SRCH_STOP_MAXITER = 5 };
enum { SRCH_ERR_NONE = 0, SRCH_ERR_NORMALS = 1 };

struct SearchState {          // the progress word the host reads one chunk behind
  int done;                   // 1: finished (a stopping rule, a covariance that stayed indefinite, or an error); later launches do nothing
  int stop;                   // SRCH_STOP_*
  int err;                    // SRCH_ERR_*
  int gen;                    // generations whose values have been consumed
  int pending;                // a generation's points are written and wait for their values
  int chol_fixed;             // generations whose C needed the 1e-14 max diag shift
  int behind;                 // launches that found the run finished
  int pad_;
  long long evals;
  double sigma, fbest, flast;
};

struct SearchArgs {
  int D, lam, mu, nh, max_iter, parity, Gmax, trace_cap;
  long long max_evals;        // <= 0: none
  unsigned long long seed;
  double cc, cs, c1, cmu, damps, chiN, mueff, tolx, tolfun, tolhistfun;
  const double *wts, *LB, *UB;        // mu, D, D
  const double* Z;                    // parity: D x lam x Gmax
  SearchState* st;
  double *xmean, *ps, *pc, *C, *A, *Y;   // D, D, D, D x D (col-major), D x D, D x lam
  double *xbest, *xlast, *hist;       // D, D, nh (ring: generation g at g % nh)
  double *Xs, *mb;                    // lam x D (col-major) points and D column means: the prediction's own buffers
  const double* F;                    // lam acquisition values of the pending generation (k_acq)
  int* tr_order;                      // trace_cap x lam   (all four may be null)
  double *tr_F, *tr_xmean, *tr_sigma; // trace_cap x lam sorted values, trace_cap x D, trace_cap
};

// The packed blocks of the search, from the shape alone (nZ: the parity normals, 0 without; tcap: trace_cap, 0 without a trace):
//   w:   wts | LB | UB | xmean ps pc xbest xlast | C | A | Y | hist | F fbar vtot | Z      (fixed: the bytes in front of Z)
//   trd: tr_F | tr_xmean | tr_sigma
// F, fbar and vtot (lam each) are what the objective's kernels write: their argument structures point into the same windows.
struct SearchBlocks {
  DevLayout w, trd;
  size_t fixed;
  DevWin<double> wts, LB, UB, xmean, ps, pc, xbest, xlast, C, A, Y, hist, F, fbar, vtot, Z, tr_F, tr_xmean, tr_sigma;
  SearchBlocks(int D, int lam, int mu, int nh, size_t nZ, size_t tcap) {
    wts = w.add<double>(mu); LB = w.add<double>(D); UB = w.add<double>(D);
    xmean = w.add<double>(D); ps = w.add<double>(D); pc = w.add<double>(D); xbest = w.add<double>(D); xlast = w.add<double>(D);
    C = w.add<double>((size_t)D * D); A = w.add<double>((size_t)D * D); Y = w.add<double>((size_t)D * lam); hist = w.add<double>(nh);
    F = w.add<double>(lam); fbar = w.add<double>(lam); vtot = w.add<double>(lam);
    fixed = w.bytes();
    Z = w.add_if<double>(nZ != 0, nZ);
    tr_F = trd.add_if<double>(tcap != 0, tcap * lam); tr_xmean = trd.add_if<double>(tcap != 0, tcap * D); tr_sigma = trd.add_if<double>(tcap != 0, tcap);
  }
  void bind(SearchArgs& a, void* dw, void* dtrd) const {
    a.wts = wts.at(dw); a.LB = LB.at(dw); a.UB = UB.at(dw); a.xmean = xmean.at(dw); a.ps = ps.at(dw); a.pc = pc.at(dw);
    a.xbest = xbest.at(dw); a.xlast = xlast.at(dw); a.C = C.at(dw); a.A = A.at(dw); a.Y = Y.at(dw); a.hist = hist.at(dw);
    a.F = F.at(dw); a.Z = Z.at(dw);
    a.tr_F = tr_F.at(dtrd); a.tr_xmean = tr_xmean.at(dtrd); a.tr_sigma = tr_sigma.at(dtrd);
  }
};

// lower Cholesky factor of the D x D matrix sC (leading dimension SRCH_MAXD + 1) into sA, column by column, lane i owning row i; every
// inner product in index order.  False: a pivot that is not positive (or not a number).  All 64 lanes call it.
__device__ __forceinline__ bool srch_chol(int D, const double* sC, double* sA, int tid) {
#pragma clang fp contract(off)
  const int LD = SRCH_MAXD + 1;
  bool ok = true;
  for (int j = 0; j < D; ++j) {
    double s = 0.0;
    if (tid >= j && tid < D) {
      s = sC[tid * LD + j];
      for (int k = 0; k < j; ++k) s = s - sA[tid * LD + k] * sA[j * LD + k];
    }
    if (tid == j) sA[j * LD + j] = s > 0.0 ? sqrt(s) : 0.0;
    __syncthreads();
    const double ajj = sA[j * LD + j];
    if (!(ajj > 0.0) || !(ajj < INFINITY)) { ok = false; break; }      // uniform: every lane reads the same word
    if (tid > j && tid < D) sA[tid * LD + j] = s / ajj;
    if (tid < j) sA[tid * LD + j] = 0.0;
    __syncthreads();
  }
  __syncthreads();
  return ok;
}

__global__ void __launch_bounds__(64) k_search_step(SearchArgs a) {
#pragma clang fp contract(off)
  const int LD = SRCH_MAXD + 1;
  __shared__ double sC[SRCH_MAXD * (SRCH_MAXD + 1)], sA[SRCH_MAXD * (SRCH_MAXD + 1)];
  __shared__ double sY[SRCH_MAXD * SRCH_MAXLAM], sF[SRCH_MAXLAM], sv[SRCH_MAXD], syw[SRCH_MAXD], spc[SRCH_MAXD], sps[SRCH_MAXD], sx[SRCH_MAXD];
  __shared__ double sred[2 * 64];
  __shared__ int sord[SRCH_MAXLAM];
  const int tid = threadIdx.x, D = a.D, lam = a.lam, mu = a.mu;
  SearchState* st = a.st;
  if (st->done) {
    if (tid == 0) st->behind = st->behind + 1;
    return;
  }
  int gen = st->gen;
  double sigma = st->sigma;
  if (st->pending) {
    // ---- rank the lambda values: not finite counts as +Inf, ties keep the index order
    if (tid < lam) { const double f = a.F[tid]; sF[tid] = (f == f && f < INFINITY && f > -INFINITY) ? f : INFINITY; }
    for (int e = tid; e < D * lam; e += 64) sY[e] = a.Y[e];
    for (int e = tid; e < D * D; e += 64) { const int i = e % D, j = e / D; sC[i * LD + j] = a.C[e]; sA[i * LD + j] = a.A[e]; }
    if (tid < D) { sx[tid] = a.xmean[tid]; spc[tid] = a.pc[tid]; sps[tid] = a.ps[tid]; }
    __syncthreads();
    if (tid < lam) {
      const double f = sF[tid];
      int r = 0;
      for (int i = 0; i < lam; ++i) { const double g = sF[i]; r += (g < f || (g == f && i < tid)) ? 1 : 0; }
      sord[r] = tid;
    }
    __syncthreads();
    const int ib = sord[0];
    const double fb = sF[ib], fw = sF[sord[lam - 1]];
    if (gen < a.trace_cap && a.tr_order) {
      if (tid < lam) { a.tr_order[(size_t)gen * lam + tid] = sord[tid]; a.tr_F[(size_t)gen * lam + tid] = sF[sord[tid]]; }
    }
    // ---- the bests: this generation's (what cmaes_modded returns as xmin / fmin) and the best ever seen
    const bool improved = fb < st->fbest;
    if (tid < D) {
      const double xb = a.Xs[ib + (size_t)lam * tid];
      a.xlast[tid] = xb;
      if (improved) a.xbest[tid] = xb;
    }
    // ---- yw = sum_k w_k y_{k:lambda}, xmean
    if (tid < D) {
      double s = 0.0;
      for (int k = 0; k < mu; ++k) s = s + a.wts[k] * sY[tid + D * sord[k]];
      syw[tid] = s;
      sx[tid] = sx[tid] + sigma * s;
    }
    __syncthreads();
    // ---- v = A^-1 yw by forward substitution (lane k keeps the k-th right-hand side)
    {
      double r = tid < D ? syw[tid] : 0.0;
      for (int i = 0; i < D; ++i) {
        if (tid == i) sv[i] = r / sA[i * LD + i];
        __syncthreads();
        if (tid > i && tid < D) r = r - sA[tid * LD + i] * sv[i];
      }
      __syncthreads();
    }
    const double cps = sqrt(a.cs * (2.0 - a.cs) * a.mueff);
    if (tid < D) sps[tid] = (1.0 - a.cs) * sps[tid] + cps * sv[tid];
    __syncthreads();
    double nps = 0.0;
    for (int d = 0; d < D; ++d) nps = nps + sps[d] * sps[d];
    nps = sqrt(nps);
    gen += 1;
    const double hs = (nps / sqrt(1.0 - pow(1.0 - a.cs, 2.0 * (double)gen)) / a.chiN < 1.4 + 2.0 / ((double)D + 1.0)) ? 1.0 : 0.0;
    if (tid < D) spc[tid] = (1.0 - a.cc) * spc[tid] + (hs * sqrt(a.cc * (2.0 - a.cc) * a.mueff)) * syw[tid];
    __syncthreads();
    const double dh = (1.0 - hs) * a.cc * (2.0 - a.cc);
    // ---- rank-one + rank-mu update of the lower triangle, mirrored: C stays exactly symmetric
    for (int e = tid; e < D * D; e += 64) {
      const int i = e % D, j = e / D;
      if (i < j) continue;
      double r = 0.0;
      for (int k = 0; k < mu; ++k) { const int c = sord[k]; r = r + (sY[i + D * c] * a.wts[k]) * sY[j + D * c]; }
      const double cij = sC[i * LD + j];
      const double v = (1.0 - a.c1 - a.cmu) * cij + a.c1 * (spc[i] * spc[j] + dh * cij) + a.cmu * r;
      a.C[i + (size_t)D * j] = v;
      a.C[j + (size_t)D * i] = v;
      if (i == j) sv[i] = v;                       // (the forward substitution is done with sv)
    }
    sigma = sigma * exp((a.cs / a.damps) * (nps / a.chiN - 1.0));
    __syncthreads();
    if (tid < D) { a.xmean[tid] = sx[tid]; a.ps[tid] = sps[tid]; a.pc[tid] = spc[tid]; }
    if (tid == 0) a.hist[(gen - 1) % a.nh] = fb;
    if (gen - 1 < a.trace_cap && a.tr_order) {
      if (tid < D) a.tr_xmean[(size_t)(gen - 1) * D + tid] = sx[tid];
      if (tid == 0) a.tr_sigma[gen - 1] = sigma;
    }
    // ---- stopping rules, in cmaes_batched's order
    const long long evals = st->evals + lam;
    bool tolx = true;
    for (int d = 0; d < D; ++d) {
      const double sd = sigma * sqrt(fmax(sv[d], 0.0));
      tolx = tolx && sd < a.tolx && sigma * fabs(spc[d]) < a.tolx;
    }
    // range of the last min(nh, gen) best values (max and min do not depend on the order)
    const int nw = gen < a.nh ? gen : a.nh;
    double hmax = -INFINITY, hmin = INFINITY;
    for (int e = tid; e < nw; e += 64) { const double h = e == (gen - 1) % a.nh ? fb : a.hist[e]; hmax = fmax(hmax, h); hmin = fmin(hmin, h); }
    sred[tid] = hmax; sred[64 + tid] = hmin;
    __syncthreads();
    hmax = -INFINITY; hmin = INFINITY;
    for (int e = 0; e < 64; ++e) { hmax = fmax(hmax, sred[e]); hmin = fmin(hmin, sred[64 + e]); }
    const double hrange = hmax - hmin;             // Inf - Inf = NaN compares false below, as in the host form
    int stop = SRCH_STOP_NONE;
    if (a.max_evals > 0 && evals >= a.max_evals) stop = SRCH_STOP_MAXFUNEVALS;
    else if (tolx) stop = SRCH_STOP_TOLX;
    else if (gen > 2 && fw - fb < a.tolfun && hrange < a.tolfun) stop = SRCH_STOP_TOLFUN;
    else if (gen > a.nh && hrange < a.tolhistfun) stop = SRCH_STOP_TOLHISTFUN;
    else if (gen >= a.max_iter) stop = SRCH_STOP_MAXITER;
    __syncthreads();
    if (tid == 0) {
      st->gen = gen; st->evals = evals; st->sigma = sigma; st->flast = fb; st->pending = 0;
      if (improved) st->fbest = fb;
      if (stop != SRCH_STOP_NONE) { st->stop = stop; st->done = 1; }
    }
    if (stop != SRCH_STOP_NONE) return;
  }
  // ---- the next generation: factorise C, sample, clamp, hand the points to the prediction
  if (a.parity && gen >= a.Gmax) {
    if (tid == 0) { st->err = SRCH_ERR_NORMALS; st->done = 1; }
    return;
  }
  __syncthreads();
  for (int e = tid; e < D * D; e += 64) { const int i = e % D, j = e / D; sC[i * LD + j] = a.C[e]; }
  if (tid < D) sx[tid] = a.xmean[tid];
  __syncthreads();
  bool ok = srch_chol(D, sC, sA, tid);
  if (!ok) {                                       // symmetric already: shift the diagonal by 1e-14 max diag, once
    double md = 0.0;
    for (int d = 0; d < D; ++d) md = fmax(md, sC[d * LD + d]);
    __syncthreads();
    if (tid < D) { const double v = sC[tid * LD + tid] + 1e-14 * md; sC[tid * LD + tid] = v; a.C[tid + (size_t)D * tid] = v; }
    __syncthreads();
    ok = srch_chol(D, sC, sA, tid);
    if (tid == 0) st->chol_fixed = st->chol_fixed + 1;
    if (!ok) {
      if (tid == 0) { st->stop = SRCH_STOP_MAXITER; st->done = 1; }
      return;
    }
  }
  for (int e = tid; e < D * lam; e += 64) {        // e = d + D j: the layout of the caller's block and of Y
    const int d = e % D, j = e / D;
    sY[e] = a.parity ? a.Z[(size_t)gen * D * lam + e] : srch_normal(a.seed, (unsigned)gen, (unsigned)j, (unsigned)d);
  }
  __syncthreads();
  for (int e = tid; e < D * lam; e += 64) {
    const int d = e % D, j = e / D;
    double y = 0.0;
    for (int k = 0; k <= d; ++k) y = y + sA[d * LD + k] * sY[k + D * j];
    double x = sx[d] + sigma * y;
    x = fmin(fmax(x, a.LB[d]), a.UB[d]);
    a.Xs[j + (size_t)lam * d] = x;
    a.Y[e] = (x - sx[d]) / sigma;
    sC[d * LD + j] = x;                            // (C is no longer needed: the points, for the means)
  }
  for (int e = tid; e < D * D; e += 64) { const int i = e % D, j = e / D; a.A[e] = sA[i * LD + j]; }
  __syncthreads();
  if (tid < D) {                                   // sq_dist's centring constant: summed over the points in order, then divided
    double s = 0.0;
    for (int j = 0; j < lam; ++j) s = s + sC[tid * LD + j];
    a.mb[tid] = s / (double)lam;
  }
  if (tid == 0) st->pending = 1;
}

// Device-resident optimisation half of gplite_train (gplite/gplite_train.m:200-306, utils/fminfill.m:101-114): the fill stage, the
// choice of the starting points and a bound-constrained quasi-Newton optimiser of gp_objfun = gplite_nlZ - gplite_hypprior, all
// driven from the device; include/vbmc_hip.h (vbmc_gp_train_optimize) describes the algorithm, tests/_trainopt_ref.py restates it.
//   k_topt_propose    the candidates of one ROUND (Nopts starts x W consecutive backtracking steps) or a chunk of the design:
//                     hyper-parameter block, noise vectors AND their derivatives (gplite_noisefun.m:176-210), Cholesky-branch
//                     scalars, hyper-prior value and gradient (gplite_hypprior.m:17-65) -- the inputs of the batched gplite_nlZ path
//   k_topt_decide     one wave per start: first accepted candidate in order, BFGS update, free set, direction, stopping tests
//   k_topt_fill_sort  MATLAB's sort of the fill values (stable, NaN last), the starts (:206,210-221,272) and widths_default (:207,258-267)
//   k_topt_close      argmin ignoring NaN, clamp, fixed coordinates (:298-306)
// Speculation: the k-th backtracking candidate clip(x + t0 2^-k d) is a function of the iterate alone, the decide kernel consumes
// candidates in order, so iterates, values, iterations and funccount are the sequential algorithm's for every W, bit for bit.
// The optimiser's own arithmetic is written with plain operators in scopes with contraction off (see slice_prop in slice_kernels.h).
#pragma once
#include "gpobj_kernels.h"

#define TOPT_MAXHYP 128
#define TOPT_MAXOPTS 16
#define TOPT_MAXW 16
#define TOPT_MAXBACK 30
static_assert(TOPT_MAXHYP >= (VBMC_LIM_D + 1) + 4 + (2 * VBMC_LIM_D + 1), "k_topt_decide keeps Nhyp doubles in LDS arrays of TOPT_MAXHYP");

// what k_topt_propose says about candidate b to k_topt_decide
enum { TOPT_VOID = 0, TOPT_EVAL = 1, TOPT_SKIP = 2, TOPT_ATX = 3, TOPT_EXHAUSTED = 4 };
// exit flags of a start
enum { TOPT_EXIT_LIMIT = 0, TOPT_EXIT_GRAD = 1, TOPT_EXIT_DF = 2, TOPT_EXIT_STEP = 3, TOPT_EXIT_LINESEARCH = -2, TOPT_EXIT_START = -3 };

struct ToptStart {      // the progress word of one start (the host reads the Nopts of them one chunk of rounds behind)
  int started;          // the evaluation at the starting point has been consumed
  int done, exitflag;
  int iterations;
  int k;                // backtracking steps of the open iteration consumed so far
  int fresh;            // the inverse-Hessian approximation is the identity (start, or reset): next update scales it first
  int stall;            // a candidate that had to be consumed failed its first (unjittered) factorisation: the host runs a checked round
  int rounds;
  long long funccount;  // evaluations the sequential algorithm needs
  long long performed;  // evaluations launched
  double f, t0;
};

struct ToptArgs : GpObjArgs {                  // (hyp .. dsn2: one row per candidate, B = max(Nopts x W, fill chunk) of them)
  int D, Nopts, W, Ninit, max_iter, hist_cap, lownoise;
  long long max_evals;
  double tol;
  const double *LB, *UB;                      // Nhyp
  const double* design;                       // Ninit x Nhyp, column-major
  ToptStart* st;                              // Nopts
  double *x, *g, *d, *H;                      // Nopts x Nhyp (x 3), Nopts x Nhyp x Nhyp
  unsigned char *act, *on;                    // B: factorise / solve this candidate
  int* code;                                  // B: TOPT_*
  const double* out;                          // [nlZ B | failure index B | dnlZ B x Nhyp] of k_nlz_final
  double *fvals, *fsorted;                    // Ninit
  int* order;                                 // Ninit, 0-based
  double* widths;                             // Nhyp
  double *hist_x, *hist_f;                    // Nopts x hist_cap x Nhyp, Nopts x hist_cap (may be null)
  int* hist_k;                                // Nopts x hist_cap: the backtracking index of the accepted candidate
  double *res_nll, *hyp_start;                // Nopts, Nhyp
  int* best;
};

// The packed blocks of vbmc_gp_train_optimize, from the shape alone (Nrows: the design's rows, BB: candidate rows):
//   in: X | y | s2 | LB UB | pmu psig pdf pc | design     ints: ptype | order | best | hist_k (one spare int behind it)
//   vec: x | g | d     lp: lp | dlp     flags: act | on     fill: fvals | fsorted | widths     res: res_nll | hyp_start
//   hist: hist_f | hist_x (absent with hist_cap = 0, when the block is one spare double)
struct ToptBlocks {
  DevLayout in, ints, vec, lp, flags, fill, res, hist;
  GpObjHead head;
  GpObjPrior prior;
  DevWin<double> LB, UB, design, x, g, d, lpv, dlp, fvals, fsorted, widths, res_nll, hyp_start, hist_f, hist_x;
  DevWin<int> ptype, order, best, hist_k;
  DevWin<unsigned char> act, on;
  ToptBlocks(int N, int D, int Nhyp, bool has_s2, int Nrows, int Nopts, int BB, int hist_cap) {
    const size_t nv = (size_t)Nopts * Nhyp, nh = (size_t)Nopts * hist_cap;
    head.add(in, N, D, has_s2);
    LB = in.add<double>(Nhyp); UB = in.add<double>(Nhyp);
    prior.add(in, Nhyp);
    design = in.add<double>((size_t)Nrows * Nhyp);
    ptype = ints.add<int>(Nhyp); order = ints.add<int>(Nrows); best = ints.add<int>(1); hist_k = ints.add<int>(nh + 1);
    x = vec.add<double>(nv); g = vec.add<double>(nv); d = vec.add<double>(nv);
    lpv = lp.add<double>(BB); dlp = lp.add<double>((size_t)BB * Nhyp);
    act = flags.add<unsigned char>(BB); on = flags.add<unsigned char>(BB);
    fvals = fill.add<double>(Nrows); fsorted = fill.add<double>(Nrows); widths = fill.add<double>(Nhyp);
    res_nll = res.add<double>(Nopts); hyp_start = res.add<double>(Nhyp);
    hist_f = hist.add_if<double>(hist_cap != 0, nh); hist_x = hist.add_if<double>(hist_cap != 0, nh * Nhyp);
    if (!hist_cap) hist.add<double>(1);
  }
  double* bind(ToptArgs& a, void* din, void* dints, void* dvec, void* dlpb, void* dflags, void* dfill, void* dres, void* dhist) const {   // returns X
    prior.bind(a, din);
    a.LB = LB.at(din); a.UB = UB.at(din); a.design = design.at(din);
    a.ptype = ptype.at(dints); a.order = order.at(dints); a.best = best.at(dints); a.hist_k = hist_k.at(dints);
    a.x = x.at(dvec); a.g = g.at(dvec); a.d = d.at(dvec);
    a.lp = lpv.at(dlpb); a.dlp = dlp.at(dlpb);
    a.act = act.at(dflags); a.on = on.at(dflags);
    a.fvals = fvals.at(dfill); a.fsorted = fsorted.at(dfill); a.widths = widths.at(dfill);
    a.res_nll = res_nll.at(dres); a.hyp_start = hyp_start.at(dres);
    a.hist_f = hist_f.at(dhist); a.hist_x = hist_x.at(dhist);
    return head.bind(a, din);
  }
};

__device__ __forceinline__ bool topt_finite(double v) { return v > -__builtin_inf() && v < __builtin_inf(); }
// min(UB - eps(UB), max(LB + eps(LB), v))   (:272,304): MATLAB's min / max pass over the NaN that eps(Inf) produces
__device__ __forceinline__ double topt_clamp_in(double v, double lb, double ub) {
#pragma clang fp contract(off)
  if (topt_finite(lb)) v = fmax(lb + matlab_eps(lb), v);
  if (topt_finite(ub)) v = fmin(ub - matlab_eps(ub), v);
  return v;
}
__device__ __forceinline__ double topt_clip(double v, double lb, double ub) { return fmin(fmax(v, lb), ub); }
__device__ __forceinline__ double topt_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// mode 1: rows c0 + b of the design (the fill stage).  mode 0: candidate j = b % W of start s = b / W.
__global__ void __launch_bounds__(256) k_topt_propose(ToptArgs a, int mode, int c0, int checked) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  if (mode == 1) {
    if (tid == 0) { a.act[b] = 1; a.on[b] = 1; }
    const int r = c0 + b;
    gpobj_emit<true>(a, b, [&](int i) { return a.design[(size_t)r + (size_t)a.Ninit * i]; });
    return;
  }
  const int s = b / a.W, j = b - s * a.W;
  const ToptStart* st = a.st + s;
  bool any_stall = false;
  for (int q = 0; q < a.Nopts; ++q) any_stall |= a.st[q].stall != 0;
  int code = TOPT_EVAL;
  double t = 0.0;
  if (st->done || (any_stall && !checked)) code = TOPT_VOID;
  else if (!st->started) code = j == 0 ? TOPT_EVAL : TOPT_SKIP;
  else if (st->k + j >= TOPT_MAXBACK) code = TOPT_EXHAUSTED;
  else t = ldexp(st->t0, -(st->k + j));
  const double *x = a.x + (size_t)s * a.Nhyp, *d = a.d + (size_t)s * a.Nhyp;
  auto cand = [&](int i) { return t == 0.0 ? x[i] : topt_clip(x[i] + t * d[i], a.LB[i], a.UB[i]); };
  if (code == TOPT_EVAL && st->started) {
    int neq = 0;
    for (int i = tid; i < a.Nhyp; i += 256) neq |= cand(i) != x[i];
    if (!__syncthreads_or(neq)) code = TOPT_ATX;
  }
  if (tid == 0) { a.code[b] = code; a.act[b] = code == TOPT_EVAL; a.on[b] = code == TOPT_EVAL; }
  if (code != TOPT_EVAL) return;                           // (workgroup-uniform)
  gpobj_emit<true>(a, b, cand);
}

// fill values of a chunk: gp_objfun, NaN for a matrix that is not positive definite after the retries (gplite_train.m:542-546)
__global__ void k_topt_fill_collect(ToptArgs a, int n, int c0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  a.fvals[c0 + b] = a.out[n + b] > 0.0 ? __builtin_nan("") : a.out[b] - a.lp[b];
}

// a before b in MATLAB's ascending sort: NaN last, ties in index order
__device__ __forceinline__ bool topt_before(double fa, int ia, double fb, int ib) {
  const bool na = fa != fa, nb = fb != fb;
  if (na != nb) return nb;
  if (na) return ia < ib;
  return fa < fb || (fa == fb && ia < ib);
}

__global__ void __launch_bounds__(256) k_topt_fill_sort(ToptArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, Ninit = a.Ninit, Nhyp = a.Nhyp, Nopts = a.Nopts;
  for (int r = tid; r < Ninit; r += 256) {
    const double fr = a.fvals[r];
    int rank = 0;
    for (int q = 0; q < Ninit; ++q) rank += topt_before(a.fvals[q], q, fr, r);
    a.order[rank] = r;
    a.fsorted[rank] = fr;
  }
  __syncthreads();
  // the starts: the best Nopts rows (:206) ...
  for (int e = tid; e < Nopts * Nhyp; e += 256) {
    const int s = e / Nhyp, i = e - s * Nhyp;
    a.x[e] = a.design[(size_t)a.order[s] + (size_t)Ninit * i];
  }
  __syncthreads();
  // ... the second one replaced by the best of the fifth of the remaining rows with the smallest noise parameter (:210-221)
  const int M = Ninit - Nopts;
  if (a.lownoise && a.Nnoise > 0 && Nopts > 1 && M > 0) {
    const int m20 = (int)ceil(0.2 * (double)M);
    __shared__ double bf[256];
    __shared__ int br[256], bq[256];
    double best_f = __builtin_nan("");
    int best_rank = 0x7fffffff, best_q = -1;
    for (int q = tid; q < M; q += 256) {
      const double pq = a.design[(size_t)a.order[Nopts + q] + (size_t)Ninit * a.Ncov];
      int rank = 0;
      for (int u = 0; u < M; ++u) {
        const double pu = a.design[(size_t)a.order[Nopts + u] + (size_t)Ninit * a.Ncov];
        rank += topt_before(pu, u, pq, q);
      }
      if (rank >= m20) continue;
      const double fq = a.fsorted[Nopts + q];
      // min over noise_y(1:m20): NaN ignored, the first of equal values; all NaN: the first element
      const bool better = best_q < 0 || (fq == fq && (best_f != best_f || fq < best_f || (fq == best_f && rank < best_rank))) ||
                          (fq != fq && best_f != best_f && rank < best_rank);
      if (better) { best_f = fq; best_rank = rank; best_q = q; }
    }
    bf[tid] = best_f; br[tid] = best_rank; bq[tid] = best_q;
    __syncthreads();
    if (tid == 0) {
      for (int u = 1; u < 256; ++u) {
        if (bq[u] < 0) continue;
        const double fq = bf[u];
        const bool better = bq[0] < 0 || (fq == fq && (bf[0] != bf[0] || fq < bf[0] || (fq == bf[0] && br[u] < br[0]))) ||
                            (fq != fq && bf[0] != bf[0] && br[u] < br[0]);
        if (better) { bf[0] = fq; br[0] = br[u]; bq[0] = bq[u]; }
      }
    }
    __syncthreads();
    const int row = a.order[Nopts + bq[0]];
    for (int i = tid; i < Nhyp; i += 256) a.x[(size_t)Nhyp + i] = a.design[(size_t)row + (size_t)Ninit * i];
    __syncthreads();
  }
  // widths_default = std(output_fill.X,[],1) (:207), zero widths repaired (:258-267)
  for (int i = tid; i < Nhyp; i += 256) {
    if (a.lownoise) {   // (Ninit > 0 in the caller's terms; the other branch's PUB - PLB stays with the caller)
      double m = 0.0, v = 0.0;
      for (int r = 0; r < Ninit; ++r) m += a.design[(size_t)r + (size_t)Ninit * i];
      m = m / (double)Ninit;
      for (int r = 0; r < Ninit; ++r) { const double t = a.design[(size_t)r + (size_t)Ninit * i] - m; v += t * t; }
      double w = Ninit > 1 ? __dsqrt_rn(v / (double)(Ninit - 1)) : 0.0;
      if (w == 0.0 && Nopts > 1) {
        m = 0.0; v = 0.0;
        for (int s = 0; s < Nopts; ++s) m += a.x[(size_t)s * Nhyp + i];
        m = m / (double)Nopts;
        for (int s = 0; s < Nopts; ++s) { const double t = a.x[(size_t)s * Nhyp + i] - m; v += t * t; }
        w = __dsqrt_rn(v / (double)(Nopts - 1));
      }
      if (w == 0.0) w = fmin(1.0, a.UB[i] - a.LB[i]);
      a.widths[i] = w;
    }
  }
  __syncthreads();
  // inside the bounds (:272); a fixed coordinate sits on its bound
  for (int e = tid; e < Nopts * Nhyp; e += 256) {
    const int i = e % Nhyp;
    const double lb = a.LB[i], ub = a.UB[i];
    a.x[e] = lb == ub ? lb : topt_clamp_in(a.x[e], lb, ub);
  }
}

// One wave per start.
__global__ void __launch_bounds__(64) k_topt_decide(ToptArgs a, int checked) {
#pragma clang fp contract(off)
  const int s = blockIdx.x, lane = threadIdx.x, W = a.W, Nhyp = a.Nhyp, B = a.Nopts * a.W, b0 = s * W;
  ToptStart* st = a.st + s;
  if (st->done || a.code[b0] == TOPT_VOID) return;
  __shared__ double x[TOPT_MAXHYP], g[TOPT_MAXHYP], sv[TOPT_MAXHYP], yv[TOPT_MAXHYP], Hy[TOPT_MAXHYP];
  double* xg = a.x + (size_t)s * Nhyp;
  double* gg = a.g + (size_t)s * Nhyp;
  double* H = a.H + (size_t)s * Nhyp * Nhyp;
  for (int i = lane; i < Nhyp; i += 64) { x[i] = xg[i]; g[i] = gg[i]; }
  __syncthreads();
  int started = st->started, done = 0, exitflag = 0, iterations = st->iterations, k = st->k, fresh = st->fresh, stall = 0;
  long long funccount = st->funccount, performed = st->performed;
  double f = st->f, t0 = st->t0, fold = 0.0;
  performed += __popcll(__ballot(lane < W && a.code[b0 + (lane < W ? lane : 0)] == TOPT_EVAL));
  const double qnan = __builtin_nan("");
  int acc_b = -1, acc_k = 0;
  bool moved = false;
  if (!started) {
    const bool pfail = a.out[B + b0] > 0.0;
    if (pfail && !checked) stall = 1;
    else {
      f = pfail ? qnan : a.out[b0] - a.lp[b0];
      funccount = 1; started = 1; k = 0; fresh = 1; iterations = 0;
      if (!topt_finite(f)) { done = 1; exitflag = TOPT_EXIT_START; }
      else acc_b = b0;
    }
  } else {
    for (int j = 0; j < W; ++j) {
      const int b = b0 + j, code = a.code[b];
      if (code == TOPT_EXHAUSTED) { done = 1; exitflag = TOPT_EXIT_LINESEARCH; break; }
      if (code == TOPT_ATX) { done = 1; exitflag = TOPT_EXIT_STEP; break; }
      if (funccount >= a.max_evals) { done = 1; exitflag = TOPT_EXIT_LIMIT; break; }
      const bool pfail = a.out[B + b] > 0.0;
      if (pfail && !checked) { stall = 1; break; }
      ++funccount;
      const double val = pfail ? qnan : a.out[b] - a.lp[b];
      const double* c = a.hyp + (size_t)b * Nhyp;
      double part = 0.0;
      for (int i = lane; i < Nhyp; i += 64) part += g[i] * (c[i] - x[i]);
      const double slope = wave_sum(part);
      if (topt_finite(val) && val <= f + 1e-4 * slope) { acc_b = b; acc_k = k; fold = f; f = val; moved = true; break; }
      ++k;
    }
  }
  if (acc_b >= 0) {
    const double* c = a.hyp + (size_t)acc_b * Nhyp;
    const double* gn = a.out + 2 * (size_t)B + (size_t)acc_b * Nhyp;
    const double* dl = a.dlp + (size_t)acc_b * Nhyp;
    if (moved) {
      double p0 = 0.0, p1 = 0.0, p2 = 0.0;
      for (int i = lane; i < Nhyp; i += 64) {
        const bool fixed = a.LB[i] == a.UB[i];
        const double si = c[i] - x[i], yi = fixed ? 0.0 : (gn[i] - dl[i]) - g[i];
        sv[i] = si; yv[i] = yi;
        p0 += si * yi; p1 += yi * yi; p2 += si * si;
      }
      const double sy = wave_sum(p0), yy = wave_sum(p1), ss = wave_sum(p2);
      __syncthreads();
      if (sy > 1e-10 * __dsqrt_rn(ss) * __dsqrt_rn(yy)) {           // the update is skipped unless s'y is safely positive
        if (fresh) {
          const double gam = sy / yy;
          for (int e = lane; e < Nhyp * Nhyp; e += 64) H[e] = (e / Nhyp == e % Nhyp) ? gam : 0.0;
          fresh = 0;
          __syncthreads();
        }
        double p3 = 0.0;
        for (int i = lane; i < Nhyp; i += 64) {
          double t = 0.0;
          for (int j = 0; j < Nhyp; ++j) t += H[(size_t)j * Nhyp + i] * yv[j];     // (H is symmetric: column i read along the lanes)
          Hy[i] = t;
          p3 += yv[i] * t;
        }
        const double yHy = wave_sum(p3), rho = 1.0 / sy, cc = rho * rho * yHy + rho;
        __syncthreads();
        for (int j = 0; j < Nhyp; ++j)
          for (int i = lane; i < Nhyp; i += 64)
            H[(size_t)j * Nhyp + i] = H[(size_t)j * Nhyp + i] - rho * (sv[i] * Hy[j] + Hy[i] * sv[j]) + cc * (sv[i] * sv[j]);
        __syncthreads();
      }
      ++iterations;
      k = 0;
    }
    for (int i = lane; i < Nhyp; i += 64) { x[i] = c[i]; g[i] = gn[i] - dl[i]; }
    __syncthreads();
    if (moved && a.hist_f && iterations <= a.hist_cap) {
      const size_t e = (size_t)s * a.hist_cap + (iterations - 1);
      for (int i = lane; i < Nhyp; i += 64) a.hist_x[e * Nhyp + i] = x[i];
      if (lane == 0) { a.hist_f[e] = f; a.hist_k[e] = acc_k; }
    }
    // stopping tests
    double pg = 0.0;
    for (int i = lane; i < Nhyp; i += 64) pg = fmax(pg, fabs(x[i] - topt_clip(x[i] - g[i], a.LB[i], a.UB[i])));
    pg = topt_wave_max(pg);
    if (pg <= a.tol) { done = 1; exitflag = TOPT_EXIT_GRAD; }
    else if (moved && fabs(f - fold) <= a.tol * (1.0 + fabs(f))) { done = 1; exitflag = TOPT_EXIT_DF; }
    else if (iterations >= a.max_iter || funccount >= a.max_evals) { done = 1; exitflag = TOPT_EXIT_LIMIT; }
    if (!done) {
      // free set from the bounds and the gradient's sign, d = -H_FF g_F
      double p0 = 0.0, p1 = 0.0;
      for (int i = lane; i < Nhyp; i += 64) {
        const double lb = a.LB[i], ub = a.UB[i];
        const bool fr = !(lb == ub) && !(x[i] <= lb && g[i] > 0.0) && !(x[i] >= ub && g[i] < 0.0);
        yv[i] = fr ? g[i] : 0.0;                      // g_F
        sv[i] = fr ? 1.0 : 0.0;
      }
      __syncthreads();
      if (!fresh) {
        for (int i = lane; i < Nhyp; i += 64) {
          double t = 0.0;
          for (int j = 0; j < Nhyp; ++j) t += H[(size_t)j * Nhyp + i] * yv[j];
          Hy[i] = sv[i] != 0.0 ? -t : 0.0;
          p0 += g[i] * Hy[i];
        }
        const double gtd = wave_sum(p0);
        if (!(gtd < 0.0)) fresh = 1;                  // not a descent direction: back to the identity
      }
      if (fresh) {
        for (int i = lane; i < Nhyp; i += 64) { Hy[i] = -yv[i]; p1 += fabs(yv[i]); }
        const double g1 = wave_sum(p1);
        t0 = fmin(1.0, 1.0 / g1);
      } else t0 = 1.0;
      double* dg = a.d + (size_t)s * Nhyp;
      for (int i = lane; i < Nhyp; i += 64) dg[i] = Hy[i];
    }
    for (int i = lane; i < Nhyp; i += 64) { xg[i] = x[i]; gg[i] = g[i]; }
  }
  if (lane == 0) {
    st->started = started; st->done = done; st->exitflag = exitflag; st->iterations = iterations; st->k = k; st->fresh = fresh;
    st->stall = stall; st->rounds = st->rounds + 1; st->funccount = funccount; st->performed = performed; st->f = f; st->t0 = t0;
  }
}

// [~,idx] = min(nll); hyp_start inside the bounds, fixed coordinates on their value (:298-306)
__global__ void __launch_bounds__(64) k_topt_close(ToptArgs a) {
  const int lane = threadIdx.x;
  int best = 0;
  double bv = __builtin_nan("");
  for (int s = 0; s < a.Nopts; ++s) {
    const double v = a.st[s].f;
    if (lane == 0) a.res_nll[s] = v;
    if (v == v && (bv != bv || v < bv)) { bv = v; best = s; }
  }
  if (lane == 0) *a.best = best;
  for (int i = lane; i < a.Nhyp; i += 64) {
    const double lb = a.LB[i], ub = a.UB[i];
    a.hyp_start[i] = lb == ub ? lb : topt_clamp_in(a.x[(size_t)best * a.Nhyp + i], lb, ub);
  }
}

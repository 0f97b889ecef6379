// The mode of the variational posterior (vbmc_mode.m) on the device: one launch optimises from every start.
//   k_vp_mode<DT>  one workgroup of MODE_W waves per start.  The objective is F(u) = logprob(u) - log q(u) in the transformed space
//                  (origflag = 0: logprob = 0), minimised by BFGS on an inverse-Hessian approximation that starts from
//                  diag((sigma_c lambda_d)^2) of the start's own component c.  The line search's candidates u + 2^-k d, k = 0 ..
//                  MODE_KMAX - 1, depend on the iterate alone: MODE_W of them are evaluated at once, one per wave, and the first in
//                  order that meets the sufficient-decrease rule is taken, which is the sequential backtracking search's outcome.
//                  Evaluation: lanes over components (component k on lane k mod 64), an online max-shifted log-sum-exp and the D
//                  gradient sums per lane, combined across the wave by xor butterflies (every lane forms the same sums in the same
//                  order: no atomics, the result depends on the inputs alone); the log-Jacobian part with lanes over dimensions.
//                  The component means are streamed from global memory (L2) in the lane-coalesced layout [d][k]; the inverse
//                  Hessian, the transform rows and the rotation live in LDS.
//                  role 1 (ranking, vbmc_mode.m:23-28): workgroup b only evaluates the objective at the mean of component b.
// The density rule of vpt_eval (log density below log(5e-324) -> -Inf) is deliberately absent: everything stays in the log domain, and
// a start far from every other component keeps a finite objective and a usable gradient.
#pragma once
#include "common.h"
#include "dev_layout.h"
#include "device_math.h"        // vb_exp_tab
#include "parity_rng.h"         // srch_log
#include "vp_tools_kernels.h"   // VptPost, VptTrS, vpt_log1p, vpt_inverse

#define MODE_W 4                       // waves per workgroup = candidates of the line search evaluated at once
#define MODE_T (64 * MODE_W)           // threads per workgroup
#define MODE_KMAX 32                   // candidates of one line search: steps 1, 1/2, .., 2^-31
#define MODE_C1 1e-4                   // sufficient decrease: F(u + t d) <= F(u) + MODE_C1 t g'd
#define MODE_CURV 1e-10                // the update is skipped unless y's > MODE_CURV |y| |s|
#define MODE_ITER_CAP 1000             // the in-kernel loop is bounded whatever the caller asks for
#define MODE_DEFAULT_ITER 200
#define MODE_DEFAULT_NMAX 20

struct ModeArgs {
  VptPost P;                 // (P.mus is not read: the means come from muT)
  const double* muT;         // DT x Kp: mu(d, k) / lambda_d at [d Kp + k]
  int Kp, origflag, max_iter, role, ranked;
  double tol_grad;
  const double* f_all;       // ranked: the objective at the K component means (what role 1 wrote)
  double* f_rank;            // role 1: K
  double *f0, *us, *xs, *fs; // S; S x D with start b at [b D ..] (us, xs)
  int *start_comp, *iters, *nfev, *stop;
};

// The two device blocks of vbmc_vp_mode, from the shape alone (S starts of K components, Kp = K rounded up to 64):
//   b: muT (DT x Kp) | f_all (K) | res        res: f0, fs (S each) | us, xs (S D each)        i: start_comp, iters, nfev, stop (S ints each)
// res and i are what the host reads back: its two vectors are images of those two layouts.
struct ModeBlocks {
  DevLayout b, res, i;
  DevWin<double> muT, f_all, f0, fs, us, xs;
  DevWin<unsigned char> results;
  DevWin<int> start_comp, iters, nfev, stop;
  ModeBlocks(int D, int DT, int K, int Kp, int S) {
    f0 = res.add<double>(S); fs = res.add<double>(S); us = res.add<double>((size_t)S * D); xs = res.add<double>((size_t)S * D);
    muT = b.add<double>((size_t)DT * Kp); f_all = b.add<double>(K); results = b.add(res);
    start_comp = i.add<int>(S); iters = i.add<int>(S); nfev = i.add<int>(S); stop = i.add<int>(S);
  }
  void bind(ModeArgs& a, void* db, void* di) const {
    void* r = results.at(db);
    a.muT = muT.at(db); a.f0 = f0.at(r); a.fs = fs.at(r); a.us = us.at(r); a.xs = xs.at(r);
    a.start_comp = start_comp.at(di); a.iters = iters.at(di); a.nfev = nfev.at(di); a.stop = stop.at(di);
  }
};

__device__ __forceinline__ double mode_wave_sum(double v) {
#pragma clang fp contract(off)
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double mode_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// v_j = sum_i (u_i scale_i) R(j, i): the coordinate before scale and rotation (warpvars_vbmc.m:285-288), in vpt_finish's order
template <int DT>
__device__ __forceinline__ double mode_unrotate(const VptPost& P, const VptTrS<DT>& S, const double* u, int j) {
#pragma clang fp contract(off)
  if (!P.has_rot) return P.has_sc ? u[j] * S.row[5][j] : u[j];
  double acc = 0.0;
  for (int i = 0; i < P.D; ++i) acc = fma(P.has_sc ? u[i] * S.row[5][i] : u[i], S.R[j * DT + i], acc);
  return acc;
}

// F and its gradient at the point uc (LDS, DT entries, zero beyond D), by ONE wave; every wave of the workgroup calls it at the same
// time with its own uc / xsc / vw / gout / fout (the barriers are the workgroup's).
template <int DT>
__device__ __forceinline__ void mode_eval(const ModeArgs& a, const VptTrS<DT>& S, const double* tab, const double* s_lam, const double* uc, double* xsc, double* vw,
                                          double* gout, double* fout, int lane) {
  const VptPost& P = a.P;
  const int D = P.D, K = P.K, Kp = a.Kp;
  if (lane < DT) xsc[lane] = lane < D ? uc[lane] / s_lam[lane] : 0.0;
  __syncthreads();
  double m = -__builtin_inf(), s = 0.0;
  double g[DT], z[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) g[d] = 0.0;
  for (int k = lane; k < K; k += 64) {
    double q = 0.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) { z[d] = xsc[d] - a.muT[(size_t)d * Kp + k]; q = fma(z[d], z[d], q); }
    const double is2 = P.is2[k];
    const double ak = fma(-0.5 * is2, q, P.cst[k]);
    // online log-sum-exp: the running maximum m and s = sum exp(a_k - m); the gradient sums carry the same shift
    const bool gt = ak > m;
    const double e = vb_exp_tab<0>(-fabs(ak - m), tab);
    s = gt ? fma(s, e, 1.0) : s + e;
    m = gt ? ak : m;
    const double sc = gt ? e : 1.0, ck = (gt ? 1.0 : e) * is2;
#pragma unroll
    for (int d = 0; d < DT; ++d) g[d] = fma(g[d], sc, ck * z[d]);
  }
  const double M = mode_wave_max(m);
  const double w = lane < K ? vb_exp_tab<0>(-fabs(m - M), tab) : 0.0;   // (a lane without a component: m = -Inf, s = 0)
  const double ssum = mode_wave_sum(s * w);
#pragma unroll
  for (int d = 0; d < DT; ++d) g[d] = d < D ? mode_wave_sum(g[d] * w) : 0.0;
  const double logq = (M + srch_log(ssum)) + P.lognf;
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < DT; ++d) gout[d] = (g[d] / ssum) * P.ilam[d];   // -d log q / d u_d
  }
  double lj = 0.0;
  if (a.origflag && P.has_tr) {
    // logprob = the log-Jacobian of warpvars_vbmc.m:463-503 (vpt_logjac + P.ljc) and its gradient, lanes over dimensions
    double term = 0.0, dv = 0.0;
    if (lane < DT) {
#pragma clang fp contract(off)
      const double v = mode_unrotate<DT>(P, S, uc, lane);
      const int t = (int)S.row[0][lane];
      if (t == 1 || t == 2) { term = v; dv = 1.0; }
      else if (t == 3) {
        const double dl = S.row[4][lane], zz = v * dl + S.row[3][lane], az = fabs(zz);
        const double e = vb_exp_tab<0>(-az, tab);
        term = -az - 2.0 * vpt_log1p(e);
        const double th = (1.0 - e) / (1.0 + e);                        // tanh(|z| / 2)
        dv = -dl * (zz < 0.0 ? -th : th);
      }
      vw[lane] = dv;
    }
    lj = mode_wave_sum(term) + P.ljc;
    __syncthreads();
    if (lane < D) {
#pragma clang fp contract(off)
      double acc;
      if (P.has_rot) {
        acc = 0.0;
        for (int i = 0; i < D; ++i) acc = fma(vw[i], S.R[i * DT + lane], acc);
      } else acc = vw[lane];
      if (P.has_sc) acc = acc * S.row[5][lane];
      gout[lane] = gout[lane] + acc;
    }
  }
  if (lane == 0) *fout = lj - logq;
  __syncthreads();
}

template <int DT>
__global__ void __launch_bounds__(MODE_T) k_vp_mode(ModeArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ VptTrS<DT> S;
  __shared__ double s_H[DT * DT];
  __shared__ double s_lam[DT], s_u[DT], s_g[DT], s_d[DT], s_s[DT], s_y[DT], s_Hy[DT];
  __shared__ double s_uc[MODE_W][DT], s_gc[MODE_W][DT], s_xs[MODE_W][DT], s_vw[MODE_W][DT], s_fc[MODE_W];
  __shared__ int s_start;
  const VptPost& P = a.P;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, D = P.D, K = P.K, b = blockIdx.x;
  for (int j = tid; j < VB_EXP_TAB_N; j += MODE_T) tab[j] = c_exp2_tab[j];
  if (P.has_tr) {
    double* rows = &S.row[0][0];
    for (int e = tid; e < VPT_NROWS * DT; e += MODE_T) rows[e] = P.tr[e];
    if (P.has_rot)
      for (int e = tid; e < DT * DT; e += MODE_T) S.R[e] = P.tr[VPT_NROWS * DT + e];
  }
  if (tid < DT) s_lam[tid] = tid < D ? P.lam[tid] : 1.0;
  if (tid == 0) s_start = b;
  __syncthreads();
  if (a.ranked) {
    // vbmc_mode.m:25-27: a stable ascending sort of -f; start b is the component that b others precede
    for (int k = tid; k < K; k += MODE_T) {
      const double fk = a.f_all[k];
      int before = 0;
      for (int j = 0; j < K; ++j) { const double fj = a.f_all[j]; before += (fj > fk || (fj == fk && j < k)) ? 1 : 0; }
      if (before == b) s_start = k;
    }
    __syncthreads();
  }
  const int c = s_start;
  const double sg = P.sig[c];
  if (tid < DT) s_u[tid] = tid < D ? P.mu[tid + (size_t)D * c] : 0.0;
  for (int e = tid; e < DT * DT; e += MODE_T) {
    const int i = e / DT, j = e - i * DT;
    const double sl = sg * s_lam[i];
    s_H[e] = (i == j && i < D) ? sl * sl : 0.0;
  }
  __syncthreads();
  if (lane < DT) s_uc[wv][lane] = s_u[lane];
  __syncthreads();
  mode_eval<DT>(a, S, tab, s_lam, s_uc[wv], s_xs[wv], s_vw[wv], s_gc[wv], &s_fc[wv], lane);
  if (a.role == 1) {
    if (tid == 0) a.f_rank[b] = -s_fc[0];
    return;
  }
  if (tid < DT) s_g[tid] = s_gc[0][tid];
  double f = s_fc[0];
  const double f0 = f;
  int iter = 0, nfev = 1, stop = VBMC_MODE_STOP_MAXITER;
  __syncthreads();
  for (;;) {
    double gmax = 0.0;
    for (int d = 0; d < D; ++d) gmax = fmax(gmax, fabs(s_g[d]));
    if (gmax <= a.tol_grad) { stop = VBMC_MODE_STOP_GRAD; break; }
    if (iter >= a.max_iter || iter >= MODE_ITER_CAP) { stop = VBMC_MODE_STOP_MAXITER; break; }
    if (tid < DT) {
#pragma clang fp contract(off)
      double acc = 0.0;
      for (int j = 0; j < D; ++j) acc = fma(s_H[tid * DT + j], s_g[j], acc);
      s_d[tid] = -acc;
    }
    __syncthreads();
    double gd = 0.0;
    for (int d = 0; d < D; ++d) gd = fma(s_g[d], s_d[d], gd);
    int take = -1;
    for (int k0 = 0; k0 < MODE_KMAX && take < 0; k0 += MODE_W) {
      if (lane < DT) s_uc[wv][lane] = lane < D ? fma(ldexp(1.0, -(k0 + wv)), s_d[lane], s_u[lane]) : 0.0;
      __syncthreads();
      mode_eval<DT>(a, S, tab, s_lam, s_uc[wv], s_xs[wv], s_vw[wv], s_gc[wv], &s_fc[wv], lane);
      nfev += MODE_W;
      for (int w = MODE_W - 1; w >= 0; --w)
        if (s_fc[w] <= fma(MODE_C1 * ldexp(1.0, -(k0 + w)), gd, f)) take = w;     // the first in order
    }
    if (take < 0) { stop = VBMC_MODE_STOP_STEP; break; }
    if (tid < DT) { s_s[tid] = s_uc[take][tid] - s_u[tid]; s_y[tid] = s_gc[take][tid] - s_g[tid]; }
    __syncthreads();
    if (tid < DT) {
#pragma clang fp contract(off)
      double acc = 0.0;
      for (int j = 0; j < D; ++j) acc = fma(s_H[tid * DT + j], s_y[j], acc);
      s_Hy[tid] = acc;
    }
    __syncthreads();
    double ys = 0.0, yHy = 0.0, ss = 0.0, yy = 0.0;
    for (int d = 0; d < D; ++d) {
      ys = fma(s_y[d], s_s[d], ys); yHy = fma(s_y[d], s_Hy[d], yHy); ss = fma(s_s[d], s_s[d], ss); yy = fma(s_y[d], s_y[d], yy);
    }
    if (ys > 0.0 && ys * ys > (MODE_CURV * MODE_CURV) * (ss * yy)) {
#pragma clang fp contract(off)
      const double rho = 1.0 / ys, c2 = rho * (1.0 + rho * yHy);
      for (int e = tid; e < DT * DT; e += MODE_T) {
        const int i = e / DT, j = e - i * DT;
        s_H[e] = (s_H[e] - rho * (s_s[i] * s_Hy[j] + s_Hy[i] * s_s[j])) + c2 * (s_s[i] * s_s[j]);
      }
    }
    f = s_fc[take];
    __syncthreads();
    if (tid < DT) { s_u[tid] = s_uc[take][tid]; s_g[tid] = s_gc[take][tid]; }
    ++iter;
    __syncthreads();
  }
  // the answer of this start; with origflag back through the inverse transform and its clamp (vpt_finish's order of operations)
  const bool back = a.origflag && P.has_tr;
  if (back && tid < DT) s_vw[0][tid] = mode_unrotate<DT>(P, S, s_u, tid);
  __syncthreads();
  if (tid == 0) {
    double x[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) x[d] = back ? s_vw[0][d] : s_u[d];
    if (back) vpt_inverse<DT>(x, S, tab);
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D) { a.us[(size_t)b * D + d] = s_u[d]; a.xs[(size_t)b * D + d] = x[d]; }
    a.fs[b] = -f; a.f0[b] = -f0; a.start_comp[b] = c; a.iters[b] = iter; a.nfev[b] = nfev; a.stop[b] = stop;
  }
}

// Step 1 of the IMIQR importance sampler and the resampling of its starting walkers on the device
// (private/activeimportancesampling_vbmc.m:106-151 and :205-215), in front of the MCMC of is_sample_kernels.h.  All randomness is an
// indexed block  B  of (D + 1) Na1 + W S doubles, Na1 = Nvp + Nbox:
//   point i < Nvp        B[0 + (D + 1) i] uniform: the component c of the 4K-component smoothed mixture by catrnd (:403-408),
//                        B[1 + d + (D + 1) i] standard normal z_d:  x_d = mu(d, c mod K) + (lambda_d sigma4_c) z_d          (vbmc_rnd.m:95)
//   point Nvp <= i < Na1 B[0 + (D + 1) i] uniform: the training input j = floor(u N),
//                        B[1 + d + (D + 1) i] uniform u_d:  x_d = X(j, d) + (2 u_d - 1) rect_delta_d                        (:140-141)
//   draw i of ensemble s B[(D + 1) Na1 + i + W s] uniform of the i-th draw without replacement                              (:210-214)
// generated (rng_mode 0) with the Philox uniforms of the slice sampler at counter (2^32 - 1, i, slot) -- the normals with the search's
// srch_normal at (2^32 - 1, i, d) -- and (2^32 - 2, s, i); the MCMC's own counters (half-move, ...) never reach those.
//   k_is_draw      one workgroup: rect_delta = 2 std(X), LB / UB (:27-31, :112), the tables of the smoothed mixture (:116-126), the points,
//                  each also into the prediction's point buffer of every ensemble
//   (k_is_pred     fmu, fs2 of the Na1 points under every hyper-sample)
//   k_is_proposal  one wave per point: the proposal's log density (:301-340 with the box terms counted) and, per hyper-sample, lnw and
//                  the resampling log weight lnw + islogf2
//   k_is_resample  one wave per hyper-sample: W draws without replacement, the chosen points clipped into the box as starting walkers
// Sums that decide a point's bits run in index order with contraction off; the exponentials and logarithms are the library's own.
#pragma once
#include "is_sample_kernels.h"

#define ISS_MAXNA VBMC_LIM_NA
#define ISS_DRAW_THREADS 256
static_assert(ISS_MAXNA <= ISS_DRAW_THREADS && ISS_MAXNA == 4 * 64, "one thread per point in k_is_draw, four weights per lane in k_is_resample");
#define ISS_CTR_POINT 0xFFFFFFFFu
#define ISS_CTR_DRAW 0xFFFFFFFEu
#define ISS_LOG_DENORM_MIN (-744.4400719213812)   // log(5e-324): the reference takes the log of a density, which is zero below it

struct IsSetupKArgs {
  int D, N, S, K, Nvp, Nbox, W, parity;
  unsigned long long seed;
  double w_vp;
  const double* X;                         // N x D column-major (the GP's)
  const double *mu, *sigma, *lambda, *w;   // D x K, K, D, K
  const double* B;                         // parity: the block
  double* geo;                             // rect_delta (D) | VV
  double *LB, *UB;                         // D each: the sampler's box
  double* comp;                            // sigma4 (4K) | cdf (4K) | cst (4K)
  double* Xa1;                             // Na1 x D column-major
  double* P;                               // S x D x Na1: the prediction's point buffer
  const double *fmu, *fs2;                 // S x Na1 (k_is_pred)
  double *lpdf, *lnw1, *fs2a1, *lw;        // Na1 | S x Nap1 | S x Nap1 | S x Na1
  double* x;                               // S x W x D: the sampler's walkers
  double* x0;                              // W x D x S: the same, as the caller reads them
  int* idx0;                               // W x S
};

// The set-up's block of fp64, from the shape alone (Na1 = Nvp + Nbox Step 1 points, Nap1 that rounded up to whole tiles of 16; W = 0
// without Step 2, when x0 still has room for one walker; parity: the caller's block B of (D + 1) Na1 + W S values, else absent):
//   mu | sigma | lambda | w | B | geo (D + 1) | comp (12 K) | Xa1 | P1 | logp fmu fs2 ys2 (S x Na1 each) | lpdf |
//   lnw1 fs2a1 (S x Nap1) | lw (S x Na1) | x0                (upload: the bytes the caller fills, mu .. B)
struct IsSetupBlock {
  DevLayout L;
  size_t upload;
  DevWin<double> mu, sigma, lambda, w, B, geo, comp, Xa1, P, logp, fmu, fs2, ys2, lpdf, lnw1, fs2a1, lw, x0;
  static size_t block_len(int D, int S, int W, int Na1) { return (size_t)(D + 1) * Na1 + (size_t)W * S; }
  IsSetupBlock(int D, int S, int K, int W, int Na1, bool parity) {
    const size_t nv1 = (size_t)S * Na1, np1 = (size_t)S * (((Na1 + 15) / 16) * 16);
    mu = L.add<double>((size_t)D * K); sigma = L.add<double>(K); lambda = L.add<double>(D); w = L.add<double>(K);
    B = L.add_if<double>(parity, block_len(D, S, W, Na1));
    upload = L.bytes();
    geo = L.add<double>(D + 1); comp = L.add<double>(12 * (size_t)K); Xa1 = L.add<double>((size_t)Na1 * D); P = L.add<double>((size_t)S * D * Na1);
    logp = L.add<double>(nv1); fmu = L.add<double>(nv1); fs2 = L.add<double>(nv1); ys2 = L.add<double>(nv1);
    lpdf = L.add<double>(Na1); lnw1 = L.add<double>(np1); fs2a1 = L.add<double>(np1); lw = L.add<double>(nv1);
    x0 = L.add<double>((size_t)(W > 1 ? W : 1) * D * S);
  }
  void bind(IsSetupKArgs& k, void* d) const {
    k.mu = mu.at(d); k.sigma = sigma.at(d); k.lambda = lambda.at(d); k.w = w.at(d); k.B = B.at(d); k.geo = geo.at(d); k.comp = comp.at(d);
    k.Xa1 = Xa1.at(d); k.P = P.at(d); k.fmu = fmu.at(d); k.fs2 = fs2.at(d); k.lpdf = lpdf.at(d); k.lnw1 = lnw1.at(d); k.fs2a1 = fs2a1.at(d);
    k.lw = lw.at(d); k.x0 = x0.at(d);
  }
  void bind(IsPredArgs& g, void* d) const { g.P = P.at(d); g.logp = logp.at(d); g.fmu = fmu.at(d); g.fs2 = fs2.at(d); g.ys2 = ys2.at(d); }   // Step 1's prediction
};

__device__ __forceinline__ double iss_u_point(const IsSetupKArgs& a, int i, int slot) {
  if (!a.parity) return slice_uniform(a.seed, ISS_CTR_POINT, (unsigned)i, (unsigned)slot);
  return a.B[(size_t)slot + (size_t)(a.D + 1) * i];
}
__device__ __forceinline__ double iss_z_point(const IsSetupKArgs& a, int i, int d) {
  if (!a.parity) return srch_normal(a.seed, ISS_CTR_POINT, (unsigned)i, (unsigned)d);
  return a.B[(size_t)(1 + d) + (size_t)(a.D + 1) * i];
}
__device__ __forceinline__ double iss_u_draw(const IsSetupKArgs& a, int s, int i) {
  if (!a.parity) return slice_uniform(a.seed, ISS_CTR_DRAW, (unsigned)s, (unsigned)i);
  return a.B[(size_t)(a.D + 1) * (a.Nvp + a.Nbox) + (size_t)i + (size_t)a.W * s];
}
__device__ __forceinline__ double iss_log(double x) { return x >= 2.2250738585072014e-308 ? srch_log(x) : -__builtin_inf(); }

__global__ void __launch_bounds__(ISS_DRAW_THREADS) k_is_draw(IsSetupKArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_wsum, s_sll;
  const int tid = threadIdx.x, D = a.D, N = a.N, K = a.K, K4 = 4 * a.K, Na1 = a.Nvp + a.Nbox;
  double *sig4 = a.comp, *cdf = a.comp + K4, *cst = a.comp + 2 * (size_t)K4;
  if (tid < D) {                                       // :27-31, :112, every sum in index order
    const double* xd = a.X + (size_t)N * tid;
    double s = 0.0, mn = xd[0], mx = xd[0];
    for (int n = 0; n < N; ++n) { const double v = xd[n]; s = s + v; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    const double mean = s / (double)N;
    double q = 0.0;
    for (int n = 0; n < N; ++n) { const double t = xd[n] - mean; q = q + t * t; }
    a.geo[tid] = 2.0 * sqrt(q / (double)(N - 1));
    const double diam = mx - mn;
    a.LB[tid] = mn - 0.5 * diam;
    a.UB[tid] = mx + 0.5 * diam;
  }
  for (int c = tid; c < K4; c += ISS_DRAW_THREADS) {   // :116-125
    const int k = c % K, r = c / K;
    const double sg = a.sigma[k], sc = r == 1 ? 0.05 : r == 2 ? 0.2 : 1.0;
    sig4[c] = r == 0 ? sg : sqrt(sg * sg + sc * sc);
  }
  __syncthreads();
  if (tid == 0) {
    double vv = 1.0, ws = 0.0, sll = 0.0;
    for (int d = 0; d < D; ++d) { vv = vv * (2.0 * a.geo[d]); sll = sll + iss_log(a.lambda[d]); }
    a.geo[D] = vv;
    for (int c = 0; c < K4; ++c) ws = ws + a.w[c % K];
    double cs = 0.0;
    for (int c = 0; c < K4; ++c) { cs = cs + a.w[c % K] / ws; cdf[c] = cs; }     // :126, catrnd's cumsum
    s_wsum = ws; s_sll = sll;
  }
  __syncthreads();
  for (int c = tid; c < K4; c += ISS_DRAW_THREADS)     // log of a component's normalisation (vbmc_pdf.m:58-63)
    cst[c] = ((iss_log(a.w[c % K] / s_wsum) - (double)D * iss_log(sig4[c])) - s_sll) - 0.5 * (double)D * 1.8378770664093453;
  if (tid >= Na1) return;
  const int i = tid;
  const double u0 = iss_u_point(a, i, 0);
  if (i < a.Nvp) {
    const double target = u0 * cdf[K4 - 1];
    int c = 0;
    for (int j = 0; j < K4; ++j) c += cdf[j] < target ? 1 : 0;
    c = min(c, K4 - 1);
    const double sg = sig4[c];
    for (int d = 0; d < D; ++d) {
      const double v = a.mu[d + (size_t)D * (c % K)] + (a.lambda[d] * sg) * iss_z_point(a, i, d);
      a.Xa1[i + (size_t)Na1 * d] = v;
      for (int s = 0; s < a.S; ++s) a.P[((size_t)s * D + d) * Na1 + i] = v;
    }
  } else {
    const int j = min((int)floor(u0 * (double)N), N - 1);
    for (int d = 0; d < D; ++d) {
      const double v = a.X[j + (size_t)N * d] + (2.0 * iss_u_point(a, i, 1 + d) - 1.0) * a.geo[d];
      a.Xa1[i + (size_t)Na1 * d] = v;
      for (int s = 0; s < a.S; ++s) a.P[((size_t)s * D + d) * Na1 + i] = v;
    }
  }
}

__device__ __forceinline__ double iss_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double iss_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// grid Nap1 (the padded rows of the state's layout), one wave each
__global__ void __launch_bounds__(64) k_is_proposal(IsSetupKArgs a) {
#pragma clang fp contract(off)
  __shared__ double tab[VB_EXP_TAB_N];
  const int i = blockIdx.x, lane = threadIdx.x, D = a.D, N = a.N, S = a.S, K = a.K, K4 = 4 * a.K, Na1 = a.Nvp + a.Nbox;
  const int Nap1 = ((Na1 + 15) / 16) * 16;
  const double ninf = -__builtin_inf();
  if (i >= Na1) {                                      // the padding of the importance-sampling state
    for (int s = lane; s < S; s += 64) { a.lnw1[(size_t)s * Nap1 + i] = ninf; a.fs2a1[(size_t)s * Nap1 + i] = 0.0; }
    return;
  }
  for (int j = lane; j < VB_EXP_TAB_N; j += 64) tab[j] = c_exp2_tab[j];
  __syncthreads();
  const double *sig4 = a.comp, *cst = a.comp + 2 * (size_t)K4;
  // ---- log density of the smoothed mixture: log-sum-exp over its 4K components
  double t0 = ninf;
  if (a.Nvp > 0) {
    double m = ninf;
    for (int c = lane; c < K4; c += 64) {
      double q = 0.0;
      for (int d = 0; d < D; ++d) { const double z = (a.Xa1[i + (size_t)Na1 * d] - a.mu[d + (size_t)D * (c % K)]) / (sig4[c] * a.lambda[d]); q = q + z * z; }
      m = fmax(m, cst[c] - 0.5 * q);
    }
    m = iss_wave_max(m);
    if (m > ninf) {
      double sum = 0.0;
      for (int c = lane; c < K4; c += 64) {
        double q = 0.0;
        for (int d = 0; d < D; ++d) { const double z = (a.Xa1[i + (size_t)Na1 * d] - a.mu[d + (size_t)D * (c % K)]) / (sig4[c] * a.lambda[d]); q = q + z * z; }
        sum = sum + vb_exp_tab<0>((cst[c] - 0.5 * q) - m, tab);
      }
      sum = iss_wave_sum(sum);
      const double lvp = m + srch_log(sum);            // (sum >= 1: the largest term is exp(0))
      if (lvp >= ISS_LOG_DENORM_MIN) t0 = lvp + srch_log(a.w_vp);             // :313
    }
  }
  // ---- the box-uniforms around the training inputs, counted (:328-333)
  double t1 = ninf;
  if (a.Nbox > 0) {
    int cnt = 0;
    for (int n = lane; n < N; n += 64) {
      bool in = true;
      for (int d = 0; d < D; ++d) in = in && fabs(a.Xa1[i + (size_t)Na1 * d] - a.X[n + (size_t)N * d]) < a.geo[d];
      cnt += in ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (cnt > 0) t1 = iss_log((double)cnt / a.geo[D] / (double)N * (1.0 - a.w_vp));
  }
  const double hi = fmax(t0, t1), lo = fmin(t0, t1);   // :335-337 in two terms
  double lpdf = ninf;
  if (hi > ninf && hi < __builtin_inf()) lpdf = lo > ninf ? hi + srch_log(1.0 + vb_exp_tab<0>(lo - hi, tab)) : hi;
  if (lane == 0) a.lpdf[i] = lpdf;
  // ---- per hyper-sample: lnw (:337, :148) and the resampling log weight lnw + islogf2 (:207)
  for (int s = lane; s < S; s += 64) {
    const double fmu = a.fmu[(size_t)s * Na1 + i], fs2 = a.fs2[(size_t)s * Na1 + i];
    double lnw = lpdf > ninf ? fmu - lpdf : ninf;
    if (!(lnw > ninf && lnw < __builtin_inf())) lnw = ninf;
    const double us = 0.6745 * sqrt(fmax(fs2, 2.2250738585072014e-308));
    double lw = lnw + (us + is_log1m(vb_exp_tab<0>(-2.0 * us, tab)));
    if (!(lnw > ninf) || !(lw > ninf && lw < __builtin_inf())) lw = ninf;
    a.lnw1[(size_t)s * Nap1 + i] = lnw;
    a.fs2a1[(size_t)s * Nap1 + i] = fs2;
    a.lw[(size_t)s * Na1 + i] = lw;
  }
}

// grid S, one wave each: lane l owns the weights 4 l .. 4 l + 3
__global__ void __launch_bounds__(64) k_is_resample(IsSetupKArgs a) {
#pragma clang fp contract(off)
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double wts[ISS_MAXNA];
  const int s = blockIdx.x, lane = threadIdx.x, D = a.D, W = a.W, Na1 = a.Nvp + a.Nbox;
  const double ninf = -__builtin_inf();
  for (int j = lane; j < VB_EXP_TAB_N; j += 64) tab[j] = c_exp2_tab[j];
  __syncthreads();
  double lw[4], m = ninf;
  for (int q = 0; q < 4; ++q) {
    const int k = 4 * lane + q;
    lw[q] = k < Na1 ? a.lw[(size_t)s * Na1 + k] : ninf;
    m = fmax(m, lw[q]);
  }
  m = iss_wave_max(m);
  for (int q = 0; q < 4; ++q) {                        // w = exp(lnw - max(lnw)) (:208); no weight at all: ones, as below
    const int k = 4 * lane + q;
    wts[k] = k >= Na1 ? 0.0 : !(m > ninf) ? 1.0 : lw[q] > ninf ? vb_exp_tab<0>(lw[q] - m, tab) : 0.0;
  }
  __syncthreads();
  for (int i = 0; i < W; ++i) {
    double p[4], incl = 0.0, total = 0.0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      double run = 0.0;
      for (int q = 0; q < 4; ++q) { run = run + wts[4 * lane + q]; p[q] = run; }
      incl = run;
      for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(incl, o, 64); if (lane >= o) incl = incl + v; }
      total = __shfl(incl, 63, 64);
      if (total > 0.0 || attempt == 1) { incl = incl - run; break; }          // (incl: now the sum of the lanes before this one)
      for (int q = 0; q < 4; ++q) wts[4 * lane + q] = 4 * lane + q < Na1 ? 1.0 : 0.0;     // the weights ran out: ones
      __syncthreads();
    }
    const double target = iss_u_draw(a, s, i) * total;   // catrnd (:403-408): idx = #(cdf < u cdf(end)) + 1
    int cnt = 0;
    for (int q = 0; q < 4; ++q) cnt += (4 * lane + q < Na1 && incl + p[q] < target) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    const int idx = min(cnt, Na1 - 1);
    __syncthreads();
    if (lane == (idx >> 2)) wts[idx] = 0.0;            // :212
    if (lane == 0) a.idx0[i + (size_t)W * s] = idx;
    if (lane < D) {
      const double v = fmin(fmax(a.Xa1[idx + (size_t)Na1 * lane], a.LB[lane]), a.UB[lane]);
      a.x[((size_t)s * W + i) * D + lane] = v;
      a.x0[i + (size_t)W * (lane + (size_t)D * s)] = v;
    }
    __syncthreads();
  }
}

// The acquisition functions behind the GP prediction (gp_pred_kernels.h): the density-based sweep k_acq, and the IQR functions on the
// importance-sampling state (k_cross_kernel, k_ctmp_pack, k_nn_noise, k_acq_iqr, k_iqr_final).
#pragma once
#include "common.h"
#include "device_math.h"

// ------------------------------------------------------------------------------------------
// Acquisition sweep (acq/acqwrapper_vbmc.m:19-46) fused behind the prediction: per test point the
// hyper-sample statistics fbar / vtot (:21-29), the variational-posterior density p = max(vbmc_pdf(vp,Xs,0),
// realmin) (vbmc_pdf.m:57-63), the acquisition value (acqf_vbmc.m:9-10, acqflog_vbmc.m:17-18, acqus_vbmc.m:9,
// acqfsn2_vbmc.m:9-17), the variance regularisation (:35-45) and the -realmax clamp (:46).
// ------------------------------------------------------------------------------------------
struct AcqArgs {
  int Nstar, S, D, K, N, acq_id, reg;
  double ymax, TolVar;
  const double* Xs;     // Nstar x D col-major
  const double* fmu;    // Nstar x S
  const double* fs2;    // Nstar x S
  const double* mu;     // D x K
  const double* isl;    // K x D:  1 / (sigma_k lambda_d)
  const double* coef;   // K:      nf * w_k / sigma_k^D
  const double* sn2x;   // Nstar   gp.sn2new at the nearest row of gp.X_rescaled (k_nn_noise)   (acq_id 3)
  double* acq;          // Nstar
  double* fbar;         // Nstar
  double* vtot;         // Nstar
};

__global__ void __launch_bounds__(256) k_acq(AcqArgs a) {
  extern __shared__ double lds[];
  const int D = a.D, K = a.K, S = a.S, Nstar = a.Nstar;
  double* s_mu = lds;              // K x D (k-major)
  double* s_isl = s_mu + K * D;    // K x D
  double* s_coef = s_isl + K * D;  // K
  for (int idx = threadIdx.x; idx < K * D; idx += 256) {
    const int k = idx / D, d = idx % D;
    s_mu[idx] = a.mu[d + (size_t)D * k];
    s_isl[idx] = a.isl[idx];
  }
  for (int k = threadIdx.x; k < K; k += 256) s_coef[k] = a.coef[k];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nstar) return;
  double fbar = 0.0, vbar = 0.0;
  for (int s = 0; s < S; ++s) { fbar += a.fmu[i + (size_t)Nstar * s]; vbar += a.fs2[i + (size_t)Nstar * s]; }
  fbar /= S; vbar /= S;
  double vf = 0.0;
  if (S > 1) {
    for (int s = 0; s < S; ++s) { const double d = a.fmu[i + (size_t)Nstar * s] - fbar; vf += d * d; }
    vf /= (S - 1);
  }
  const double vtot = vf + vbar;
  double x[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) x[d] = d < D ? a.Xs[i + (size_t)Nstar * d] : 0.0;
  double p = 0.0;
  for (int k = 0; k < K; ++k) {
    double d2 = 0.0;
#pragma unroll
    for (int d = 0; d < 32; ++d)
      if (d < D) { const double t = (x[d] - s_mu[k * D + d]) * s_isl[k * D + d]; d2 = fma(t, t, d2); }
    p += s_coef[k] * exp(-0.5 * d2);
  }
  p = fmax(p, 2.2250738585072014e-308);
  double acq;
  if (a.acq_id == 0) acq = -vtot * exp(fbar - a.ymax) * p;
  else if (a.acq_id == 1) acq = -(log(vtot) + fbar - a.ymax + log(p));
  else if (a.acq_id == 2) acq = -vtot * p * p;
  else {
    const double sn2 = a.sn2x[i];   // observation noise at the nearest training input (k_nn_noise; acqfsn2_vbmc.m:11-13)
    acq = -vtot * (1.0 - sn2 / (vtot + sn2)) * exp(fbar - a.ymax) * p;
  }
  if (a.reg && vtot < a.TolVar) {
    if (a.acq_id == 1) acq = acq + a.TolVar / vtot - 1.0;
    else acq = acq * exp(-(a.TolVar / vtot - 1.0));
  }
  acq = fmax(acq, -1.7976931348623157e308);
  a.acq[i] = acq;
  if (a.fbar) a.fbar[i] = fbar;
  if (a.vtot) a.vtot[i] = vtot;
}

// ------------------------------------------------------------------------------------------
// Importance-sampled IQR acquisition functions (acq/acqviqr_vbmc.m:50-109, acq/acqimiqr_vbmc.m:40-95) and the
// Step-3 precomputation of private/activeimportancesampling_vbmc.m:248-276.
// ------------------------------------------------------------------------------------------
// Kax'[s] (N x Na, column a at a*N): k_s(X_n, Xa_a)  (:264-265)
__global__ void __launch_bounds__(256) k_cross_kernel(int N, int D, int Nhyp, int Na, int per_s, const double* __restrict__ X,
                                                      const double* __restrict__ Xa /* Na x D (x S) col-major */,
                                                      const double* __restrict__ hyp, double* __restrict__ Z) {
  const int s = blockIdx.y;
  const double* h = hyp + (size_t)s * Nhyp;
  __shared__ double iell[32];
  if (threadIdx.x < D) iell[threadIdx.x] = 1.0 / exp(h[threadIdx.x]);
  __syncthreads();
  const double sf2 = exp(2.0 * h[D]);
  const double* xa = Xa + (per_s ? (size_t)s * Na * D : 0);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < (size_t)N * Na; idx += (size_t)gridDim.x * 256) {
    const int n = (int)(idx % N), a = (int)(idx / N);
    double c = 0.0;
    for (int d = 0; d < D; ++d) { const double t = (X[n + (size_t)N * d] - xa[a + (size_t)Na * d]) * iell[d]; c = fma(t, t, c); }
    Z[(size_t)s * N * Na + idx] = sf2 * exp(-c / 2.0);
  }
}

// CtmpT[s][n][a] (a fastest, padded to Nap with zeros) = U[s][a*N + n] / sn2_eff (Lchol, :271) or U (else, :273)
__global__ void __launch_bounds__(256) k_ctmp_pack(int N, int Na, int Nap, const double* __restrict__ U,
                                                   const double* __restrict__ sn2_eff, const unsigned char* __restrict__ lchol,
                                                   double* __restrict__ CT) {
  const int s = blockIdx.y;
  const double sc = lchol[s] ? 1.0 / sn2_eff[s] : 1.0;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < (size_t)N * Nap; idx += (size_t)gridDim.x * 256) {
    const int a = (int)(idx % Nap), n = (int)(idx / Nap);
    CT[(size_t)s * N * Nap + idx] = a < Na ? U[(size_t)s * N * Na + (size_t)a * N + n] * sc : 0.0;
  }
}

// observation noise at the nearest training input in length-scale units (acqviqr_vbmc.m:42-43); first minimum wins.
// One wave per 16 test points; the inner products of |x - xr_n|^2 = |x|^2 + |xr_n|^2 - 2 x.xr_n for 16 x 16 blocks of
// (training point, test point) pairs are QS MFMAs, each lane then scans its four candidates in increasing n.
template <int QS>
__global__ void __launch_bounds__(64) k_nn_noise(int Nstar, int N, int D, const double* __restrict__ Xs, const double* __restrict__ gl,
                                                 const double* __restrict__ Xr, const double* __restrict__ sn2new,
                                                 double* __restrict__ sn2x) {
  const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
  const int i = blockIdx.x * 16 + li;
  const int gi = min(i, Nstar - 1);
  double xb[QS];                                   // B operand: test point li, dimensions 4q + lg
#pragma unroll
  for (int q = 0; q < QS; ++q) {
    const int d = 4 * q + lg;
    xb[q] = d < D ? Xs[gi + (size_t)Nstar * d] / gl[d] : 0.0;
  }
  double best = INFINITY;
  int pos = 0;
  for (int n0 = 0; n0 < N; n0 += 16) {
    const int na = min(n0 + li, N - 1);            // A operand: training point n0 + li, dimensions 4q + lg
    vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
    double rr = 0.0;
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int d = 4 * q + lg;
      const double av = d < D ? Xr[na + (size_t)N * d] : 0.0;
      rr = fma(av, av, rr);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xb[q], acc, 0, 0, 0);
    }
    rr += __shfl_xor(rr, 16, 64);                  // |xr_n|^2 for n = n0 + li, on every lane group
    rr += __shfl_xor(rr, 32, 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int nl = lg + 4 * r, n = n0 + nl;       // accumulator row
      const double rn = __shfl(rr, nl, 64);         // |xr_n|^2 lives on lane li == nl
      const double c = rn - 2.0 * acc[r];           // + |x|^2, the same for every n
      if (n < N && c < best) { best = c; pos = n; }
    }
  }
  // the four lane groups hold disjoint n: smallest distance, ties to the smaller index
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int op = __shfl_xor(pos, o, 64);
    if (ob < best || (ob == best && op < pos)) { best = ob; pos = op; }
  }
  if (lg == 0 && i < Nstar) sn2x[i] = sn2new[pos];
}

struct IqrArgs {
  int N, D, S, Nhyp, Nstar, Na, Nap, per_s;
  const double* Xs;      // Nstar x D col-major
  const double* Xa;      // Na x D (x S) col-major
  const double* hyp;     // Nhyp x S
  const double* Xc;      // S x N x D   ell-scaled, centred training inputs (k_pred_prep)
  const double* muv;     // S x 2D      centre, 1/ell
  const double* CT;      // S x N x Nap
  const double* fs2a;    // S x Nap
  const double* lnw;     // S x Nap (-inf in the padding) or null
  const double* fs2;     // Nstar x S   (k_gp_pred)
  const double* KsW;     // S x ceil(Nstar/16) x N x 16  sW-scaled cross-kernel matrix, tiled by 16 points (k_pred_ks)
  const double* sn2_eff; // S
  const double* sn2x;    // Nstar
  const unsigned char* lchol;
  double* acqs;          // Nstar x S
};

// One workgroup = 4 waves = 64 test points x one hyper-sample; wave w owns 16 of the points.
// C[i][a] = Ka[i][a] -/+ sum_n Ks[n][i] Ctmp[n][a] on the fp64 matrix cores: the A operand Ks[n][i] comes from the
// cross-kernel matrix k_pred_ks left in memory (one coalesced value per lane and k-step); the B operand -- rows of CtmpT,
// the same for all points -- is staged through LDS in chunks of 16 rows shared by its waves (double-buffered: the
// global loads of chunk c+1 are in flight while chunk c feeds the MFMAs), which divides the L2 traffic of the B stream by
// IQR_WPB; NT = Nap/16 accumulator tiles live at once.
// Epilogue per element: tau2 = C^2/ys2_i, s_pred = sqrt(max(fs2a_a - tau2, 0)), zz = lnw_a + u s + log1p(-exp(-2 u s)),
// then a log-sum-exp over a (16 lanes x NT tiles).
#define IQR_KC 16
#define IQR_WPB 8                       // waves (16-point tiles) per workgroup
#define IQR_PTS (16 * IQR_WPB)
#define IQR_THREADS (64 * IQR_WPB)
#define IQR_LDS_BYTES(NT) ((size_t)(2 * IQR_KC * (16 * (NT) + 8) + IQR_PTS * 33 + IQR_PTS) * sizeof(double))
template <int NT>
__global__ void __launch_bounds__(IQR_THREADS) k_acq_iqr(IqrArgs a) {
  constexpr int BS = 16 * NT + 8;          // padded row stride of a staged chunk
  constexpr int PER = (IQR_KC * 16 * NT + IQR_THREADS - 1) / IQR_THREADS;   // staged elements per thread
  extern __shared__ double iq_lds[];
  double* BL = iq_lds;                              // [2][IQR_KC][BS]
  double (*xs_s)[33] = (double (*)[33])(iq_lds + 2 * IQR_KC * BS);   // ell-scaled, centred test points of the workgroup's points
  double* ys2_s = iq_lds + 2 * IQR_KC * BS + IQR_PTS * 33;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int ib = blockIdx.x * IQR_PTS, i0 = ib + 16 * wv, s = blockIdx.y;
  const int N = a.N, D = a.D, Nap = a.Nap;
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  const double sf2 = exp(2.0 * h[D]);
  const double* mu = a.muv + (size_t)s * 2 * D;
  const double* iell = mu + D;
  for (int idx = tid; idx < IQR_PTS * D; idx += IQR_THREADS) {
    const int i = idx / D, d = idx % D;
    const int gi = min(ib + i, a.Nstar - 1);
    xs_s[i][d] = a.Xs[gi + (size_t)a.Nstar * d] * iell[d] - mu[d];
  }
  if (tid < IQR_PTS) {
    const int gi = min(ib + tid, a.Nstar - 1);
    ys2_s[tid] = a.fs2[gi + (size_t)a.Nstar * s] + a.sn2x[gi];
  }
  vb_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (vb_d4){0.0, 0.0, 0.0, 0.0};
  const double* ct = a.CT + (size_t)s * N * Nap;
  const bool gvalid = i0 + li < a.Nstar;
  const double* kcol = a.KsW + ((size_t)s * ((a.Nstar + 15) >> 4) + (i0 >> 4)) * (size_t)N * 16 + li;   // [s][point tile][n][16]
  const double isw = a.lchol[s] ? sqrt(a.sn2_eff[s]) : 1.0;   // undo sW = 1/sqrt(sn2_eff)
  // chunk c = rows 16c .. 16c+15 of CtmpT (contiguous in memory: row-major N x Nap), zero beyond N
  double pre[PER];
  auto fetch = [&](int c) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + IQR_THREADS * u;
      pre[u] = (e < IQR_KC * Nap && 16 * c * Nap + e < N * Nap) ? ct[(size_t)16 * c * Nap + e] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + IQR_THREADS * u;
      if (e < IQR_KC * Nap) { const int row = e / Nap, col = e - row * Nap; BL[(buf * IQR_KC + row) * BS + col] = pre[u]; }
    }
  };
  const int nch = (N + IQR_KC - 1) / IQR_KC;
  // A operands of the four k-steps of a chunk: the cross-kernel values k_s(X_n, xs_i) (stored sW-scaled), loaded one
  // chunk ahead like the B rows
  double kv[4], kvn[4], kvn2[4];   // this chunk, the next one and the one after (the A stream comes from HBM)
  auto fetch_a = [&](int c, double* dst) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 16 * c + 4 * q + lg;
      dst[q] = (n < N && gvalid) ? kcol[(size_t)n * 16] : 0.0;
    }
  };
  fetch(0);
  fetch_a(0, kv);
  fetch_a(1, kvn);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int cur = c & 1;
    if (c + 1 < nch) fetch(c + 1);
    fetch_a(c + 2, kvn2);
#pragma unroll
    for (int q = 0; q < 4; ++q) kv[q] *= isw;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double* brow = BL + (cur * IQR_KC + 4 * q + lg) * BS + li;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[q], brow[16 * t], acc[t], 0, 0, 0);
    }
    if (c + 1 < nch) stash(cur ^ 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) { kv[q] = kvn[q]; kvn[q] = kvn2[q]; }
    __syncthreads();
  }
  const int xo = 16 * wv;   // this wave's rows of xs_s / ys2_s
  // the staged chunks are no longer needed: the exp table takes their place
  double* TAB = BL;
  for (int t = tid; t < VB_EXP_TAB_N; t += IQR_THREADS) TAB[t] = c_exp2_tab[t];
  // ... and the ell-scaled, centred importance points XA[d][a] (each is needed by 4 lanes of every wave)
  double* XA = BL + VB_EXP_TAB_N;
  const double* xa = a.Xa + (a.per_s ? (size_t)s * a.Na * D : 0);
  const bool xa_lds = (size_t)(VB_EXP_TAB_N + D * Nap) <= (size_t)2 * IQR_KC * BS;
  if (xa_lds)
    for (int e = tid; e < D * Nap; e += IQR_THREADS) {
      const int d = e / Nap, aa_ = e - d * Nap;
      XA[e] = aa_ < a.Na ? xa[aa_ + (size_t)a.Na * d] * iell[d] - mu[d] : 0.0;
    }
  __syncthreads();
  // epilogue: lane (li, lg) holds C'[i = lg + 4r][a = 16t + li]
  const double u = 0.6745;
  const double sgn = a.lchol[s] ? -1.0 : 1.0;
  double zz[NT][4];
  double mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int aa_ = 16 * t + li;
    const bool av = aa_ < a.Na;
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d) {
      const double xv = xa_lds ? XA[d * Nap + aa_] : (av ? xa[aa_ + (size_t)a.Na * d] * iell[d] - mu[d] : 0.0);
#pragma unroll
      for (int r = 0; r < 4; ++r) { const double tt = xs_s[xo + lg + 4 * r][d] - xv; c4[r] = fma(tt, tt, c4[r]); }
    }
    const double fa = av ? a.fs2a[(size_t)s * Nap + aa_] : 0.0;
    const double lw = av ? (a.lnw ? a.lnw[(size_t)s * Nap + aa_] : 0.0) : -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = lg + 4 * r;
      const double ka = sf2 * vb_exp_tab<0>(-0.5 * c4[r], TAB);
      const double C = ka + sgn * acc[t][r];
      const double tau2 = C * C / ys2_s[xo + i];
      const double sp = sqrt(fmax(fa - tau2, 0.0));
      const double z = av ? lw + (u * sp + log1p(-vb_exp_tab<0>(-2.0 * u * sp, TAB))) : -INFINITY;
      zz[t][r] = z;
      mx[r] = fmax(mx[r], z);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double m = mx[r];
    m = fmax(m, __shfl_xor(m, 1, 64)); m = fmax(m, __shfl_xor(m, 2, 64));
    m = fmax(m, __shfl_xor(m, 4, 64)); m = fmax(m, __shfl_xor(m, 8, 64));
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) sum += vb_exp_tab<0>(zz[t][r] - m, TAB);
    sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64); sum += __shfl_xor(sum, 8, 64);
    const int gi = i0 + lg + 4 * r;
    // every term -inf: MATLAB's -inf - -inf = NaN propagates (the table exp itself swallows NaN)
    if (li == 0 && gi < a.Nstar) a.acqs[gi + (size_t)a.Nstar * s] = (m == -INFINITY) ? NAN : log(sum) + m;
  }
}

// acq = M + log(sum(exp(acq_s - M))/Ns) over hyper-samples (:104-107), then the log-flag variance regulariser and the
// clamp of acq/acqwrapper_vbmc.m:35-46; also fbar / vtot (:21-29)
__device__ __forceinline__ void iqr_final_point(int i, int Nstar, int S, int reg, double TolVar, const double* acqs, const double* fmu,
                                                const double* fs2, double* acq, double* fbar_o, double* vtot_o) {
  double fbar = 0.0, vbar = 0.0;
  for (int s = 0; s < S; ++s) { fbar += fmu[i + (size_t)Nstar * s]; vbar += fs2[i + (size_t)Nstar * s]; }
  fbar /= S; vbar /= S;
  double vf = 0.0;
  if (S > 1) {
    for (int s = 0; s < S; ++s) { const double d = fmu[i + (size_t)Nstar * s] - fbar; vf += d * d; }
    vf /= (S - 1);
  }
  const double vtot = vf + vbar;
  double v;
  if (S > 1) {
    double M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmax(M, acqs[i + (size_t)Nstar * s]);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += exp(acqs[i + (size_t)Nstar * s] - M);
    v = M + log(sum / S);
  } else v = acqs[i];
  if (reg && vtot < TolVar) v = v + TolVar / vtot - 1.0;
  v = fmax(v, -1.7976931348623157e308);
  acq[i] = v;
  if (fbar_o) fbar_o[i] = fbar;
  if (vtot_o) vtot_o[i] = vtot;
}

__global__ void __launch_bounds__(256) k_iqr_final(int Nstar, int S, int reg, double TolVar, const double* __restrict__ acqs,
                                                   const double* __restrict__ fmu, const double* __restrict__ fs2,
                                                   double* __restrict__ acq, double* __restrict__ fbar_o, double* __restrict__ vtot_o) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nstar) return;
  iqr_final_point(i, Nstar, S, reg, TolVar, acqs, fmu, fs2, acq, fbar_o, vtot_o);
}

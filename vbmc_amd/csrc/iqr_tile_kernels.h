// The IQR acquisition functions (acq/acqviqr_vbmc.m:36-109, acq/acqimiqr_vbmc.m:30-95) for ONE tile of at most 16 points: the
// objective of the device-resident acquisition search on noisy targets (vbmc_acq_search_iqr).  k_acq_iqr (gp_acq_kernels.h) is shaped for
// sweeps of thousands of points -- eight waves of 16 points each, every wave walking all ceil(N / 16) chunks of Ctmp behind a workgroup
// barrier; with the search's lambda <= 16 points seven of its waves are idle and the grid is S workgroups.  Here the work of the one
// tile is split the other way:
//   grid (NT, S): one workgroup per 16 importance points (tile t of Nap / 16) and hyper-sample;
//   its W <= 8 waves split the sum over the N training points: wave w takes the 16-row chunks w, w + W, ... of
//     C[i][a] = Ka[i][a] -/+ sum_n Ks[n][i] Ctmp[n][a]                      (v_mfma_f64_16x16x4_f64, fp64 throughout)
//   A operand: the sW-scaled cross-kernel tile the prediction left (k_pred_ks: [s][n][16]); B operand: rows of the state's CT
//   ([s][n][Nap]).  Both are read straight from memory -- every value is needed by exactly one lane of one wave -- so the loop has no
//   LDS traffic and no barrier; the dependent chain per hyper-sample is ceil(N / (16 W)) chunk steps.
//   The waves' partial tiles are added through LDS in wave order, then wave 0 runs k_acq_iqr's epilogue on the 16 x 16 tile and
//   leaves, per point, the record (max, sum of exp(z - max)) of its 16 importance points.
//   k_iqr_tile_final combines the NT records of a point in tile order into the log-sum-exp per hyper-sample and closes with
//   k_iqr_final's step (log-mean-exp over hyper-samples, fbar / vtot, the regulariser and the clamp).
// Every sum runs in a fixed order (W is a function of N alone), nothing is atomic: two runs give the same bits, and a point's value
// depends neither on its slot nor on the other slots (an MFMA output element is a function of its own row and column).
// Slots lam .. 15 are padding: their indices are clamped, their A operands are zero and their records are not written.
#pragma once
#include "common.h"
#include "device_math.h"
#include "gp_acq_kernels.h"   // IqrArgs, iqr_final_point

#define IQRT_MAXW 8
#define IQRT_LDS_BYTES(W) ((size_t)(W) * 256 * sizeof(double))

struct IqrTileArgs {
  int N, D, S, Nhyp, lam, Na, Nap, per_s, reg;
  double TolVar;
  const double* Xs;      // lam x D col-major (k_search_step)
  const double* Xa;      // Na x D (x S) col-major
  const double* hyp;     // Nhyp x S
  const double* muv;     // S x 2D      centre, 1/ell (k_pred_prep)
  const double* CT;      // S x N x Nap
  const double* fs2a;    // S x Nap
  const double* lnw;     // S x Nap (-inf in the padding) or null
  const double* fmu;     // lam x S
  const double* fs2;     // lam x S
  const double* KsW;     // S x N x 16  sW-scaled cross-kernel tile (k_pred_ks)
  const double* sn2_eff; // S
  const double* sn2x;    // lam (k_nn_noise)
  const unsigned char* lchol;
  double* rec;           // S x NT x 16 x 2: (max, sum) per point and importance-point tile
  double* acqs;          // lam x S
  double *acq, *fbar, *vtot;   // lam each: acq is where k_search_step reads the generation's values
};

__global__ void __launch_bounds__(64 * IQRT_MAXW) k_acq_iqr_tile(IqrTileArgs a) {
  extern __shared__ double it_part[];                 // [W][4][64] partial accumulators
  __shared__ double xs_s[16][33], ys2_s[16], TAB[VB_EXP_TAB_N];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int W = blockDim.x >> 6, t = blockIdx.x, s = blockIdx.y;
  const int N = a.N, D = a.D, Nap = a.Nap, lam = a.lam;
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  const double* mu = a.muv + (size_t)s * 2 * D;
  const double* iell = mu + D;
  // staged for the epilogue (read behind the barrier below): the ell-scaled, centred points, fs2 + sn2x and the exp table
  for (int idx = tid; idx < 16 * D; idx += blockDim.x) {
    const int i = idx / D, d = idx % D;
    const int gi = min(i, lam - 1);
    xs_s[i][d] = a.Xs[gi + (size_t)lam * d] * iell[d] - mu[d];
  }
  if (tid < 16) {
    const int gi = min(tid, lam - 1);
    ys2_s[tid] = a.fs2[gi + (size_t)lam * s] + a.sn2x[gi];
  }
  for (int e = tid; e < VB_EXP_TAB_N; e += blockDim.x) TAB[e] = c_exp2_tab[e];
  const double* ct = a.CT + (size_t)s * N * Nap + 16 * t + li;   // column 16 t + li of CtmpT
  const double* kcol = a.KsW + (size_t)s * N * 16 + li;         // point li of the cross-kernel tile
  const bool pvalid = li < lam;
  const double isw = a.lchol[s] ? sqrt(a.sn2_eff[s]) : 1.0;      // undo sW = 1/sqrt(sn2_eff)
  const int nch = (N + 15) >> 4;
  vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
  double kv[4], bv[4], kvn[4], bvn[4];                           // this wave's chunk and its next one, loaded one step ahead
  auto fetch = [&](int c, double* k, double* b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 16 * c + 4 * q + lg;
      const bool ok = c < nch && n < N;
      const size_t nn = ok ? (size_t)n : 0;                      // clamped: a chunk beyond the end loads row 0 and uses zeros
      const double kx = kcol[nn * 16], bx = ct[nn * Nap];
      k[q] = (ok && pvalid) ? kx : 0.0;
      b[q] = ok ? bx : 0.0;
    }
  };
  fetch(wv, kv, bv);
  for (int c = wv; c < nch; c += W) {
    fetch(c + W, kvn, bvn);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[q] * isw, bv[q], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { kv[q] = kvn[q]; bv[q] = bvn[q]; }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) it_part[(wv * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (wv != 0) return;
  double tot[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) tot[r] = it_part[r * 64 + lane];
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[r] += it_part[(w * 4 + r) * 64 + lane];
  // epilogue: lane (li, lg) holds C'[i = lg + 4r][a = 16t + li]
  const double u = 0.6745;
  const double sf2 = exp(2.0 * h[D]);
  const double sgn = a.lchol[s] ? -1.0 : 1.0;
  const int aa_ = 16 * t + li;
  const bool av = aa_ < a.Na;
  const int ac = min(aa_, a.Na - 1);
  const double* xa = a.Xa + (a.per_s ? (size_t)s * a.Na * D : 0);
  double c4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int d = 0; d < D; ++d) {
    const double xv = xa[ac + (size_t)a.Na * d] * iell[d] - mu[d];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const double tt = xs_s[lg + 4 * r][d] - xv; c4[r] = fma(tt, tt, c4[r]); }
  }
  const double fa = av ? a.fs2a[(size_t)s * Nap + aa_] : 0.0;
  const double lw = av ? (a.lnw ? a.lnw[(size_t)s * Nap + aa_] : 0.0) : -INFINITY;
  double* rec = a.rec + ((size_t)s * gridDim.x + t) * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = lg + 4 * r;
    const double ka = sf2 * vb_exp_tab<0>(-0.5 * c4[r], TAB);
    const double C = ka + sgn * tot[r];
    const double tau2 = C * C / ys2_s[i];
    const double sp = sqrt(fmax(fa - tau2, 0.0));
    const double z = av ? lw + (u * sp + log1p(-vb_exp_tab<0>(-2.0 * u * sp, TAB))) : -INFINITY;
    double m = z;
    m = fmax(m, __shfl_xor(m, 1, 64)); m = fmax(m, __shfl_xor(m, 2, 64));
    m = fmax(m, __shfl_xor(m, 4, 64)); m = fmax(m, __shfl_xor(m, 8, 64));
    double sum = (z == -INFINITY) ? 0.0 : vb_exp_tab<0>(z - m, TAB);
    sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64); sum += __shfl_xor(sum, 8, 64);
    if (li == 0 && i < lam) { rec[2 * i] = m; rec[2 * i + 1] = sum; }
  }
}

// the NT records of a point in tile order -> the log-sum-exp over the importance points per hyper-sample (NaN when every term is
// -inf: MATLAB's -inf - -inf), then k_iqr_final's closing step.  One thread per point.
__global__ void __launch_bounds__(64) k_iqr_tile_final(IqrTileArgs a, int NT) {
  const int i = threadIdx.x;
  if (i >= a.lam) return;
  for (int s = 0; s < a.S; ++s) {
    const double* rec = a.rec + (size_t)s * NT * 32 + 2 * i;
    double M = -INFINITY;
    for (int t = 0; t < NT; ++t) M = fmax(M, rec[(size_t)t * 32]);
    double sum = 0.0;
    for (int t = 0; t < NT; ++t) {
      const double m = rec[(size_t)t * 32];
      if (m != -INFINITY) sum += rec[(size_t)t * 32 + 1] * exp(m - M);
    }
    a.acqs[i + (size_t)a.lam * s] = (M == -INFINITY) ? NAN : log(sum) + M;
  }
  iqr_final_point(i, a.lam, a.S, a.reg, a.TolVar, a.acqs, a.fmu, a.fs2, a.acq, a.fbar, a.vtot);
}

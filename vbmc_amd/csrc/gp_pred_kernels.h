// gplite GP surrogate on gfx950, prediction and Bayesian quadrature: predictive mean / variance from the posterior of
// gp_factor_kernels.h.
//
// Reference: gplite/gplite_pred.m:52-165, gplite/gplite_quad.m:1-119, gplite/gplite_post.m:210-216.
//
//   k_pred_prep     ell-scaled, sq_dist-centred training inputs per hyper-sample
//   k_gp_pred       four waves per 16 test points: cross-kernel slab -> fmu = m* + Ks'alpha, V = inv(L')*(sW.*Ks) as
//                   MFMA products against the precomputed triangular inverse, fs2 = kss - |V|^2
//   k_pred_avg      hyper-sample averaging with between-sample variance (gplite_pred.m:154-165)
//   k_quad_*        the Bayesian-quadrature forms of the prediction kernels (gplite_quad.m): inputs scaled by 1/sqrt(sigma^2 + ell^2),
//                   the normaliser lnnf in the exponent, nf_kk and the integrated mean function in the closing step
//   k_gp_ks         the cross-covariance column of the rank-one append
#pragma once
#include "common.h"
#include "device_math.h"
#include "gp_factor_kernels.h"   // gp_meanfun
#include "trsm_mfma.h"           // tmf4

// ------------------------------------------------------------------------------------------
// Prediction: one wave = 16 test points x one hyper-sample.
// ------------------------------------------------------------------------------------------
struct PredArgs {
  int N, D, S, Nhyp, Nstar, meanfun, moff, noff, nf0, nf1, nf2;
  int mc;                // weight m of mean(b) in sq_dist's centring constant: Nstar; 0 centres on the training inputs alone, so that
                         // a point's prediction does not depend on the batch it is evaluated in (the IQR acquisition search)
  const double* X;       // N x D
  const double* Xs;      // Nstar x D (column-major)
  const double* s2s;     // Nstar or null
  const double* ys;      // Nstar or null: ystar, only for the output-dependent noise term
  const double* hyp;     // Nhyp x S
  const double* alpha;   // N x S
  const double* L;       // N x N x S
  const double* sn2_eff; // S  (1/sW^2)
  const double* sn2_mult;// S
  const unsigned char* lchol;
  const double* mean_a;  // D  column means of X
  const double* mean_b;  // D  column means of Xstar
  const double* finv;    // S x nblk x 256 inverse diagonal blocks (k_diag_inv)
  const double* tinv;    // S x N x N  inv(L') per Lchol sample, element (row, col) at col*N + row
  double* fmu;           // Nstar x S
  double* fs2;
  double* ys2;
  // Bayesian quadrature (gplite_quad.m; null for prediction): Xs holds the means mu_i of the Gaussians N(mu_i, diag sigma^2)
  const double* qsig;    // D      the shared row sigma
  double* qnf;           // S x 2  ln of the cross normaliser lnnf_s (:71) and nf_kk,s (:99), written by k_quad_prep
};

// k_pred_prep: per hyper-sample the ell-scaled, sq_dist-centred training inputs and their squared norms:
// Xc[s][i][d] = X(i,d)/ell_d - mu_d,  aa[s][i] = |Xc_i|^2,  mu = (m/(n+m)) mean(b) + (n/(n+m)) mean(a)  (sq_dist.m:36)
// QUAD (k_quad_prep): the scale is 1/tau_d, tau_d = sqrt(sigma_d^2 + ell_d^2) (gplite_quad.m:70,74) -- the kernels downstream read it
// where they read 1/ell -- and the two normalisers lnnf = ln sf2 + sum ln ell - sum ln tau (:71) and
// nf_kk = exp(ln sf2 + sum ln ell - sum ln sqrt(2 sigma^2 + ell^2)) (:98-99) go to qnf[s][0..1]
template <bool QUAD>
__device__ __forceinline__ void pred_prep_body(const PredArgs& a, double* __restrict__ Xc, double* __restrict__ aa, double* __restrict__ muv) {
  const int s = blockIdx.y, N = a.N, D = a.D;
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  __shared__ double mu[32], iell[32];
  if (threadIdx.x < D) {
    const int d = threadIdx.x;
    double ie;
    if constexpr (QUAD) {
      const double el = exp(h[d]);
      ie = 1.0 / sqrt(fma(a.qsig[d], a.qsig[d], el * el));   // 1 ./ tau   (gplite_quad.m:70)
    } else {
      ie = 1.0 / exp(h[d]);   // diag(1./ell) * X'   (gplite_pred.m:73)
    }
    const double n = (double)N, m = (double)a.mc;
    iell[d] = ie;
    mu[d] = (m / (n + m)) * (a.mean_b[d] * ie) + (n / (n + m)) * (a.mean_a[d] * ie);
    if (blockIdx.x == 0) { muv[(size_t)s * 2 * D + d] = mu[d]; muv[(size_t)s * 2 * D + D + d] = ie; }
  }
  if constexpr (QUAD) {
    if (blockIdx.x == 0 && threadIdx.x == 64) {   // O(D), in the reference's order of summation
      double sl = 0.0, st = 0.0, sk = 0.0;
      for (int d = 0; d < D; ++d) {
        const double el2 = exp(h[d]) * exp(h[d]), sg2 = a.qsig[d] * a.qsig[d];
        sl += h[d];
        st += log(sqrt(sg2 + el2));
        sk += log(sqrt(2.0 * sg2 + el2));
      }
      a.qnf[2 * s] = 2.0 * h[D] + sl - st;
      a.qnf[2 * s + 1] = exp(2.0 * h[D] + sl - sk);
    }
  }
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
      double v = a.X[i + (size_t)N * d] * iell[d] - mu[d];
      Xc[((size_t)s * N + i) * D + d] = v;
      acc = fma(v, v, acc);
    }
    aa[(size_t)s * N + i] = acc;
  }
}
__global__ void __launch_bounds__(256) k_pred_prep(PredArgs a, double* __restrict__ Xc, double* __restrict__ aa,
                                                   double* __restrict__ muv /* S x 2D: mu, 1/ell */) {
  pred_prep_body<false>(a, Xc, aa, muv);
}
__global__ void __launch_bounds__(256) k_quad_prep(PredArgs a, double* __restrict__ Xc, double* __restrict__ aa,
                                                   double* __restrict__ muv /* S x 2D: mu, 1/tau */) {
  pred_prep_body<true>(a, Xc, aa, muv);
}

// k_pred_ks: the sW-scaled cross-kernel matrix for every hyper-sample, KsW[s][i/16][n][i%16] = sW_s * k_s(X_n, Xstar_i)
// (tiled by 16 points), each element computed exactly once, and fmu's data term Ks' alpha (gplite_pred.m:74,83).
// One wave per (16 test points, hyper-sample).  The inner products of sq_dist's expansion |a|^2 + |b|^2 - 2 a.b
// (sq_dist.m:45) for a 16 x 16 block of (training point, test point) pairs are QS MFMAs (inner dimension D in steps
// of 4); the accumulator layout (row n = lg + 4 reg, column point = li) is exactly the coalesced store pattern.
// QUAD (k_quad_ks): the same pass over the tau-scaled inputs of k_quad_prep with ln of the normaliser lnnf_s in place of ln sf2:
// z = exp(lnnf - sumdelta2 / 2) (gplite_quad.m:72-76), F's data term z * alpha (:77)
template <int QS, bool QUAD>
__device__ __forceinline__ void pred_ks_body(const PredArgs& a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                             const double* __restrict__ muv, double* __restrict__ KsW, double* __restrict__ partF) {
  __shared__ double tab[VB_EXP_TAB_N];
  const int pt = blockIdx.x, s = blockIdx.y, lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
  const int N = a.N, D = a.D;
  for (int t = lane; t < VB_EXP_TAB_N; t += 64) tab[t] = c_exp2_tab[t];
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  const double* mu = muv + (size_t)s * 2 * D;
  const double* iell = mu + D;
  const double sf2 = exp(2.0 * h[D]);
  const double lsf2 = QUAD ? a.qnf[2 * s] : 2.0 * h[D];
  const double sW = a.lchol[s] ? 1.0 / sqrt(a.sn2_eff[s]) : 1.0;
  const int jc = pt * 16 + li;
  const bool cv = jc < a.Nstar;
  // B operand: this lane's test point li, dimensions 4q + lg; |b|^2 of the point by a 4-lane-group reduction
  double xb[QS];
  double bb = 0.0;
#pragma unroll
  for (int q = 0; q < QS; ++q) {
    const int d = 4 * q + lg;
    xb[q] = (d < D && cv) ? a.Xs[jc + (size_t)a.Nstar * d] * iell[d] - mu[d] : 0.0;
    bb = fma(xb[q], xb[q], bb);
  }
  bb += __shfl_xor(bb, 16, 64);
  bb += __shfl_xor(bb, 32, 64);
  __syncthreads();
  const double* al = a.alpha + (size_t)s * N;
  const double* xcs = Xc + (size_t)s * N * D;
  const double* aas = aa + (size_t)s * N;
  // tiled layout KsW[s][point tile][n][16]: each 16-point tile is one contiguous N x 16 block, written here and streamed by
  // k_gp_pred / k_acq_iqr front to back (a row-major N x Nstar matrix made every consumer hop 8 * Nstar bytes per step)
  double* out = KsW + ((size_t)s * gridDim.x + pt) * (size_t)N * 16;
  double fm = 0.0;
  (void)sf2;
  for (int n0 = 0; n0 < N; n0 += 16) {
    // A operand: training point n0 + li, dimensions 4q + lg
    const int na = min(n0 + li, N - 1);
    vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int d = 4 * q + lg;
      const double av = d < D ? xcs[(size_t)na * D + d] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xb[q], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + lg + 4 * r;
      if (n < N) {
        const double cdist = fmax(aas[n] + (bb - 2.0 * acc[r]), 0.0);      // sq_dist.m:45,49
        const double ks = vb_exp_tab<0>(lsf2 - cdist / 2.0, tab);          // sf2 * exp(-K/2)  (gplite_pred.m:74)
        fm = fma(ks, al[n], fm);
        if (cv) out[(size_t)n * 16 + li] = ks * sW;                        // sW .* Ks (:99); plain Ks when !Lchol
      }
    }
  }
  fm += __shfl_xor(fm, 16, 64);
  fm += __shfl_xor(fm, 32, 64);
  if (lg == 0 && cv) partF[(size_t)s * a.Nstar + jc] = fm;
}
template <int QS>
__global__ void __launch_bounds__(64) k_pred_ks(PredArgs a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                                const double* __restrict__ muv, double* __restrict__ KsW, double* __restrict__ partF) {
  pred_ks_body<QS, false>(a, Xc, aa, muv, KsW, partF);
}
template <int QS>
__global__ void __launch_bounds__(64) k_quad_ks(PredArgs a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                                const double* __restrict__ muv, double* __restrict__ KsW, double* __restrict__ partF) {
  pred_ks_body<QS, true>(a, Xc, aa, muv, KsW, partF);
}

// k_gp_pred: V = L' \ (sW .* Ks) as the product Tinv * (sW .* Ks), Tinv = inv(L') precomputed once per GP
// (k_trsm_fwd on the identity; |inv(L')| <= 1 because L'L = K/sl + I >= I, so the explicit inverse is as well
// conditioned as the substitution).  The operand that is REUSED is made resident:
//   * a workgroup owns a block of up to 8 consecutive 16-row tiles of Tinv (rows [r0, r1), columns [0, r1): lower
//     triangle), as large as one CU's LDS allows (156 KB), and keeps it there for its whole life;
//   * its 16 waves stream over (a z-slice of) the test-point tiles: per k-step (4 training points) a lane reads ONE cross-kernel value
//     of k_pred_ks's matrix (the MFMA B operand, coalesced over the 16 points, two steps ahead) and issues one MFMA per
//     resident row tile (A from LDS);
//   * per point tile it writes sum_rows V^2 to a partial slot; k_pred_final adds the partials in block order:
//     fs2 = kss - sum(V.^2) (gplite_pred.m:99-100).
// Low-noise samples (Lchol = false, L = -inv(K + sn2 I), :103-104) use single-tile blocks over all columns and
// accumulate Ks .* (L*Ks) instead.  Tinv / L are read from HBM/L2 once per workgroup, not once per point tile.
#define PRED_THREADS 1024
#define PRED_MAXG 80
#define PRED_MAXR 8
#define PRED_LDS_MAX (156 * 1024)
// group table (ints): ng[s] at [s]; t0 at [S + s*PRED_MAXG + g]; t1 at [S + S*PRED_MAXG + s*PRED_MAXG + g]
// One point tile against RR resident row tiles: sum over the rows of V^2 (Lchol) or Ks .* (L Ks) (low-noise samples).
// The B operand (one cross-kernel value per lane and k-step, coalesced over the 16 points) is loaded four k-steps
// ahead of its MFMAs; the A operands come from the LDS-resident block T[col][row].
template <int RR>
__device__ __forceinline__ double pred_tile(const double* __restrict__ T, int RB, const double* __restrict__ kcol, size_t ldk, int N,
                                            int ncol, bool cv, bool lc, int tb, int li, int lg) {
  tmf4 acc[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = (tmf4){0.0, 0.0, 0.0, 0.0};
  auto ldb = [&](int n0) { const int n = n0 + lg; return (cv && n < N && n0 < ncol) ? kcol[(size_t)n * ldk] : 0.0; };
  double bq[4] = {ldb(0), ldb(4), ldb(8), ldb(12)};
  for (int n0 = 0; n0 < ncol; n0 += 16) {
    double bn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) bn[u] = ldb(n0 + 16 + 4 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (n0 + 4 * u < ncol) {
        const double* trow = T + (size_t)(n0 + 4 * u + lg) * RB + li;
#pragma unroll
        for (int r = 0; r < RR; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(trow[16 * r], bq[u], acc[r], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) bq[u] = bn[u];
  }
  // C layout: lane (col = li = point, row = lg + 4 reg) of each resident tile
  double part = 0.0;
  if (lc) {
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fma(acc[r][q], acc[r][q], part);   // sum(V.*V)
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {                                            // sum(Ks .* (L*Ks)), one row tile per block
      const int row = tb * 16 + lg + 4 * q;
      const double kv = (cv && row < N) ? kcol[(size_t)row * ldk] : 0.0;
      part = fma(kv, acc[0][q], part);
    }
  }
  return part;
}

__global__ void __launch_bounds__(PRED_THREADS, 4) k_gp_pred(PredArgs a, const double* __restrict__ KsW, const int* __restrict__ grp,
                                                             double* __restrict__ partV /* G x S x Nstar */) {
  extern __shared__ double lds[];
  const int g = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  if (g >= grp[s]) return;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int N = a.N;
  const int tb = grp[a.S + s * PRED_MAXG + g], te = grp[a.S + a.S * PRED_MAXG + s * PRED_MAXG + g];
  const int R = te - tb;                       // resident row tiles
  const int RB = R * 16;                       // resident rows
  const bool lc = a.lchol[s] != 0;
  const int Np = ((N + 15) >> 4) << 4;
  const int ncol = lc ? te * 16 : Np;          // columns that matter (lower triangle / full)
  double* T = lds;                             // ncol x RB: T[col * RB + row_local]
  const double* Am = (lc ? a.tinv : a.L) + (size_t)s * N * N;   // element (row, col) at col*N + row
  for (int idx = tid; idx < ncol * RB; idx += PRED_THREADS) {
    const int col = idx / RB, rl = idx % RB, row = tb * 16 + rl;
    T[idx] = (col < N && row < N) ? Am[(size_t)col * N + row] : 0.0;
  }
  __syncthreads();
  const int ntile = (a.Nstar + 15) >> 4;
  const double* ksw = KsW + (size_t)s * ntile * N * 16;   // [point tile][n][16]
  for (int pt = wave + (PRED_THREADS / 64) * blockIdx.z; pt < ntile; pt += (PRED_THREADS / 64) * gridDim.z) {
    const int jc = pt * 16 + li;
    const bool cv = jc < a.Nstar;
    const double* kcol = ksw + (size_t)pt * N * 16 + li;
    double part = 0.0;
    switch (R) {   // one straight-line instantiation per number of resident row tiles
#define PRED_CASE(RR) case RR: part = pred_tile<RR>(T, RB, kcol, (size_t)16, N, ncol, cv, lc, tb, li, lg); break;
      PRED_CASE(1) PRED_CASE(2) PRED_CASE(3) PRED_CASE(4) PRED_CASE(5) PRED_CASE(6) PRED_CASE(7) PRED_CASE(8)
#undef PRED_CASE
      default: break;
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (lg == 0 && cv) partV[((size_t)g * a.S + s) * a.Nstar + jc] = part;
  }
}

// k_pred_fused (round 6): gplite_pred's variance WITHOUT the cross-kernel matrix in memory (gplite_pred.m:74-104).  k_pred_ks wrote
// sW .* Ks for every (hyper-sample, training point, test point) -- 524 MB at N* = 8192, S = 20, N = 400 -- and every row group of
// k_gp_pred streamed its columns of it again (2.2 GB against ~16 MB of inputs and outputs).  Here the roles of the two operands are
// swapped: a workgroup computes the N x 16 cross-kernel tiles of PT point tiles ONCE, into LDS (each value exactly once on the whole
// device: the distances as QS MFMAs per 16 x 16 block and the table exponential, as k_pred_ks), and its sixteen waves then walk the
// row tiles of inv(L') -- 640 KB per hyper-sample at N = 400, read through the L2 (the workgroups in flight share one or two
// hyper-samples: x fastest in the grid) -- with every A operand loaded once per k-step and used against the PT resident tiles.
// Row tiles are dealt to the waves in snake order over the four SIMD classes (tile b costs b + 1 k-steps x 4: the sums per SIMD, not
// per wave, are what the matrix pipe sees).  Low-noise samples (Lchol = false, :103-104) take all columns and accumulate
// Ks .* (L Ks).  fmu's data term Ks' alpha (:83) is a dot product over the resident tile.  Partial sums: one per hyper-sample and
// point (block 0 of partV; k_pred_final is told there is one block).
// dynamic LDS: PT x Np x 16 doubles (beside 2 KB of table and NWV x PT x 16 doubles of per-wave sums), and at least the
// NWV x PREDF_MAXPT x 16 doubles of the variance's per-wave sums, which reuse the block once the tiles are dead: PREDF_LDS_BYTES.
#define PREDF_THREADS 768      // twelve waves, three per SIMD (168 registers: sixteen at 128 spilled 37; eight left the matrix pipe half idle behind the L2)
#define PREDF_MAXPT 3
// resident point tiles the registers allow at QS dim-blocks (168 registers at three waves per SIMD; beyond: spills -- tests/test_lane_build.py)
#define PREDF_PT_FOR_QS(QS_) ((QS_) <= 3 ? 3 : ((QS_) <= 5 ? 2 : 1))
// QUAD (k_quad_fused): the quadrature form (gplite_quad.m:70-77,96-105) is the same pass with the tau-scaled inputs of k_quad_prep and
// ln of the normaliser lnnf_s in place of ln sf2: the tile value is z, the sums are sum V^2 with V = L' \ (sW .* z') and sum z .* (L z').
#define PREDF_LDS_BYTES(PT_, NP_) (std::max((size_t)(PT_) * (NP_) * 16, (size_t)(PREDF_THREADS / 64) * PREDF_MAXPT * 16) * sizeof(double))
template <int QS, int PT, bool QUAD>
__device__ __forceinline__ void pred_fused_body(const PredArgs& a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                                const double* __restrict__ muv, double* __restrict__ partV,
                                                double* __restrict__ partF, const int RS) {
  // RS > 1 (few points: the units do not cover the chip): RS workgroups share a unit -- each computes the unit's tiles (cheap) and takes
  // every RS-th row tile of inv(L'); their partial sums are blocks rs of partV, which k_pred_final adds in block order.  The importance
  // sampler's predictions of ~110 points were 60 workgroups walking 25 row tiles each: 74 us a call, 187 dependent calls.
  constexpr int NWV = PREDF_THREADS / 64;
  extern __shared__ double KsL[];              // [p][n][16], sW-scaled, zero for n >= N and for points beyond Nstar
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double FMW[NWV][PT][16];          // fmu's data term per wave (its row blocks), added in wave order
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int N = a.N, D = a.D, Np = ((N + 15) >> 4) << 4, nblk = Np >> 4;
  const int ntile = (a.Nstar + 15) >> 4, npass = (ntile + PT - 1) / PT, nunit = npass * a.S * RS;
  for (int t = tid; t < VB_EXP_TAB_N; t += PREDF_THREADS) tab[t] = c_exp2_tab[t];
  __syncthreads();
  // A workgroup's LDS is full -- two never share a compute unit -- so the grid is one workgroup per unit of the chip, each walking the
  // units (hyper-sample, pass) b, b + gridDim.x, ...: what a workgroup does once (launch, table) is paid once, the test points of the
  // next unit are in flight behind the current one, and at any moment the workgroups in flight share one or two hyper-samples' factors
  for (int unit = blockIdx.x; unit < nunit; unit += gridDim.x) {
    const int rs = unit % RS, u2 = unit / RS;
    const int s = u2 / npass, pass = u2 - s * npass;
    const int pt0 = pass * PT;
    const int npt = min(PT, ntile - pt0);
    const double* h = a.hyp + (size_t)s * a.Nhyp;
    const double* mu = muv + (size_t)s * 2 * D;
    const double* iell = mu + D;
    const double lsf2 = QUAD ? a.qnf[2 * s] : 2.0 * h[D];
    const bool lc = a.lchol[s] != 0;
    const double sW = lc ? 1.0 / sqrt(a.sn2_eff[s]) : 1.0;
    const double* xcs = Xc + (size_t)s * N * D;
    const double* aas = aa + (size_t)s * N;
    const double* al = a.alpha + (size_t)s * N;
    const double* Am = (lc ? a.tinv : a.L) + (size_t)s * N * N;   // element (row, col) at col * N + row
    const __amdgpu_buffer_rsrc_t Ar = __builtin_amdgcn_make_buffer_rsrc((void*)Am, 0, (int)((size_t)N * N * 8), 0x00020000);
    // ---- the cross-kernel tiles: 16 x 16 blocks (training points n0 .. n0 + 15 x the tile's points).  A wave takes the row blocks
    // n0 = 16 (wave + NWV i) of EVERY resident point tile; the training-point fragment, |a|^2 and alpha of a row block are loaded once per
    // block and one block ahead; fmu's data term Ks' alpha (:83) is accumulated on the way
    {
      double xb[PT][QS], bb[PT], fmacc[PT];
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        const bool cv = p < npt && (pt0 + p) * 16 + li < a.Nstar;
        bb[p] = 0.0; fmacc[p] = 0.0;
#pragma unroll
        for (int q = 0; q < QS; ++q) {
          const int d = 4 * q + lg;
          xb[p][q] = (cv && d < D) ? fma(a.Xs[(pt0 + p) * 16 + li + (size_t)a.Nstar * d], iell[d], -mu[d]) : 0.0;
          bb[p] = fma(xb[p][q], xb[p][q], bb[p]);
        }
        bb[p] = xor_sum16(bb[p]);
        bb[p] = xor_sum32(bb[p]);
      }
      auto ld_a = [&](int nb, double (&av)[QS], double (&an)[4]) {
        const int n0 = nb * 16, na = min(n0 + li, N - 1);
#pragma unroll
        for (int q = 0; q < QS; ++q) { const int d = 4 * q + lg; av[q] = (d < D && nb < nblk) ? xcs[(size_t)na * D + d] : 0.0; }
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int n = n0 + lg + 4 * r; an[r] = (n < N && nb < nblk) ? aas[n] : 0.0; }
      };
      double av[QS], an[4];
      ld_a(wave, av, an);
      for (int nb = wave; nb < nblk; nb += NWV) {
        double avn[QS], ann[4], ah[4];
        ld_a(nb + NWV, avn, ann);
        const int n0 = nb * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int n = n0 + lg + 4 * r; ah[r] = n < N ? al[n] : 0.0; }     // (alpha: consumed after the exponentials)
#pragma unroll
        for (int p = 0; p < PT; ++p) {
          vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int q = 0; q < QS; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], xb[p][q], acc, 0, 0, 0);
          const bool cv = p < npt && (pt0 + p) * 16 + li < a.Nstar;
          double* out = KsL + ((size_t)p * Np + n0) * 16;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = n0 + lg + 4 * r;
            double v = 0.0;
            if (n < N && cv) {
              const double cdist = fmax(an[r] + (bb[p] - 2.0 * acc[r]), 0.0);      // sq_dist.m:45,49
              v = vb_exp_tab<0>(lsf2 - cdist / 2.0, tab);                          // sf2 exp(-K/2)  (gplite_pred.m:74)
            }
            fmacc[p] = fma(v, ah[r], fmacc[p]);
            out[(lg + 4 * r) * 16 + li] = v * sW;                                  // sW .* Ks  (:99)
          }
        }
#pragma unroll
        for (int q = 0; q < QS; ++q) av[q] = avn[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) an[r] = ann[r];
      }
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        double fm = xor_sum16(fmacc[p]);
        fm = xor_sum32(fm);
        if (lg == 0) FMW[wave][p][li] = fm;
      }
    }
    __syncthreads();
    if (tid < npt * 16) {
      const int p = tid >> 4, i = tid & 15, jc = (pt0 + p) * 16 + i;
      double fm = 0.0;
      for (int w = 0; w < NWV; ++w) fm += FMW[w][p][i];
      if (jc < a.Nstar && rs == 0) partF[(size_t)s * a.Nstar + jc] = fm;
    }
    // ---- the product: this wave's row tiles against the PT resident tiles
    double part[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) part[p] = 0.0;
    for (int k0 = rs; k0 < nblk; k0 += RS) {
      // this workgroup's row tiles k0 = rs, rs + RS, .. (descending cost); the i-th of them -> SIMD class in snake order, wave within the class in turn
      const int k = k0 / RS;
      const int kq = k & 7, cls = kq < 4 ? kq : 7 - kq, wsel = cls + 4 * ((k >> 2) % (NWV / 4));
      if (wsel != wave) continue;
      const int rt = nblk - 1 - k0;
      const int ncol = lc ? (rt + 1) * 16 : Np;
      const int row = rt * 16 + li;
      const bool rv = row < N;
      tmf4 acc[PT];
#pragma unroll
      for (int p = 0; p < PT; ++p) acc[p] = (tmf4){0.0, 0.0, 0.0, 0.0};
      // Operands in chunks of four k-steps, BOTH loaded one chunk ahead of their MFMAs into two register sets used in turn: the A operands
      // (inv(L'), from the L2) and the B operands (the resident tiles, from LDS).  The scheduling barriers keep the next chunk's loads
      // ABOVE the current chunk's MFMAs: left to itself the compiler sank half of the global loads and every LDS read down to right in
      // front of their consumers (s_waitcnt vmcnt / lgkmcnt directly ahead of every second MFMA: half of the waves' cycles were such
      // waits, SQ_WAIT_INST_ANY in profiles/r06_aux.md).
      // (A through a buffer descriptor: base and extent in scalar registers, ONE 32-bit offset per lane and a scalar add per load -- the
      // 64-bit address, the compare and the select per element were 3 VALU instructions per MFMA of this loop, and on this chip every VALU
      // instruction of a SIMD waits while an fp64 MFMA executes.  Columns beyond N lie past the extent and read 0; the lanes of rows
      // beyond N start 2 GB up and stay past it)
      const unsigned vo = rv ? (unsigned)(((size_t)row + (size_t)lg * N) * 8) : 0x80000000u;
      const double* bl = KsL + (size_t)lg * 16 + li;
      auto lda4 = [&](int c0, double (&d)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          d[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(Ar, (int)(vo + (unsigned)((c0 + 4 * u) * N * 8)), 0, 0));
      };
      auto ldb4 = [&](int c0, double (&b)[4][PT]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < PT; ++p) b[u][p] = bl[(size_t)(c0 + 4 * u) * 16 + (size_t)p * Np * 16];
      };
      auto mm4 = [&](const double (&d)[4], const double (&b)[4][PT]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < PT; ++p) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(d[u], b[u][p], acc[p], 0, 0, 0);
      };
      double a0[4], a1[4], q0[4][PT], q1[4][PT];
      lda4(0, a0);
      ldb4(0, q0);
      for (int c0 = 0; c0 < ncol; c0 += 32) {
        const bool two = c0 + 16 < ncol;
        if (two) { lda4(c0 + 16, a1); ldb4(c0 + 16, q1); }
        __builtin_amdgcn_sched_barrier(0);
        mm4(a0, q0);
        if (two) {
          if (c0 + 32 < ncol) { lda4(c0 + 32, a0); ldb4(c0 + 32, q0); }
          __builtin_amdgcn_sched_barrier(0);
          mm4(a1, q1);
        }
      }
      // C layout: lane (col = li = point, row = rt * 16 + lg + 4 q)
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        if (lc) {
#pragma unroll
          for (int q = 0; q < 4; ++q) part[p] = fma(acc[p][q], acc[p][q], part[p]);     // sum(V .* V)          (:100)
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)                                                   // sum(Ks .* (L * Ks))  (:104)
            part[p] = fma(KsL[((size_t)p * Np + rt * 16 + lg + 4 * q) * 16 + li], acc[p][q], part[p]);
        }
      }
    }
    // ---- the waves' partial sums, added in wave order (the tiles' LDS is dead: it holds them)
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PT; ++p) {
      double v = xor_sum16(part[p]);
      v = xor_sum32(v);
      if (lg == 0) KsL[(wave * PREDF_MAXPT + p) * 16 + li] = v;
    }
    __syncthreads();
    if (tid < npt * 16) {
      const int p = tid >> 4, i = tid & 15, jc = (pt0 + p) * 16 + i;
      double v = 0.0;
      for (int w = 0; w < NWV; ++w) v += KsL[(w * PREDF_MAXPT + p) * 16 + i];
      if (jc < a.Nstar) partV[((size_t)rs * a.S + s) * a.Nstar + jc] = v;
    }
    __syncthreads();      // the next unit writes the tiles
  }
}
template <int QS, int PT>
__global__ void __launch_bounds__(PREDF_THREADS, 1) k_pred_fused(PredArgs a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                                                 const double* __restrict__ muv, double* __restrict__ partV,
                                                                 double* __restrict__ partF, const int RS) {
  pred_fused_body<QS, PT, false>(a, Xc, aa, muv, partV, partF, RS);
}
template <int QS, int PT>
__global__ void __launch_bounds__(PREDF_THREADS, 1) k_quad_fused(PredArgs a, const double* __restrict__ Xc, const double* __restrict__ aa,
                                                                 const double* __restrict__ muv, double* __restrict__ partV,
                                                                 double* __restrict__ partF, const int RS) {
  pred_fused_body<QS, PT, true>(a, Xc, aa, muv, partV, partF, RS);
}

// k_pred_slab: the large-N form of the prediction variance (N beyond what k_gp_pred keeps resident: a 16-row tile of the
// triangular inverse no longer fits the LDS).  One wave per CW test points: their sW-scaled cross-kernel columns form a slab
// in LDS, V = L' \ (sW .* Ks) by the blocked substitution of trsm_mfma.h (gplite_pred.m:99), sum(V.^2) per point (:100);
// low-noise samples (L = -inv(K + sn2 I)) accumulate Ks .* (L * Ks) (:103-104) with lanes along the rows.  Writes block
// partial 0 (k_pred_final is told there is one block per hyper-sample).
template <int CW>
__global__ void __launch_bounds__(64) k_pred_slab(PredArgs a, const double* __restrict__ KsW, double* __restrict__ partV) {
  extern __shared__ double lds[];
  const int cb = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const int N = a.N, Np = ((N + 15) >> 4) << 4;
  const int ntile = (a.Nstar + 15) >> 4;
  const int j0 = cb * CW;                       // first test point of the slab
  double* V = lds;
  double* P = V + (size_t)Np * (CW + 1);
  const double* ksw = KsW + (size_t)s * ntile * N * 16;   // [point tile][n][16]
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + c;
    const double* col = ksw + (size_t)(j >> 4) * N * 16 + (j & 15);
    for (int i = lane; i < Np; i += 64) V[i * (CW + 1) + c] = (j < a.Nstar && i < N) ? col[(size_t)i * 16] : 0.0;
  }
  trsm_wsync();
  if (a.lchol[s]) {
    trsm_fwd_wave<CW>(N, a.L + (size_t)s * N * N, a.finv + (size_t)s * TRSM_NBLK(N) * 256, V, P, lane);
    for (int c = 0; c < CW; ++c) {
      double part = 0.0;
      for (int i = lane; i < N; i += 64) { const double v = V[i * (CW + 1) + c]; part = fma(v, v, part); }
      part = wave_sum(part);
      if (lane == 0 && j0 + c < a.Nstar) partV[(size_t)s * a.Nstar + j0 + c] = part;
    }
  } else {
    const double* Lm = a.L + (size_t)s * N * N;    // symmetric: element (i, j) at j * N + i
    for (int c = 0; c < CW; ++c) {
      double part = 0.0;
      for (int i = lane; i < N; i += 64) {
        double acc = 0.0;
        for (int j = 0; j < N; ++j) acc = fma(Lm[(size_t)j * N + i], V[j * (CW + 1) + c], acc);
        part = fma(V[i * (CW + 1) + c], acc, part);
      }
      part = wave_sum(part);
      if (lane == 0 && j0 + c < a.Nstar) partV[(size_t)s * a.Nstar + j0 + c] = part;
    }
  }
}

// fmu = m* + Ks' alpha (:83), fs2 = max(kss -/+ sum of the block partials, 0) (:100,:104,:120), ys2 (:121)
__global__ void __launch_bounds__(256) k_pred_final(PredArgs a, const int* __restrict__ grp, const double* __restrict__ partV,
                                                    const double* __restrict__ partF) {
  const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= a.Nstar) return;
  const int D = a.D;
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  const double sf2 = exp(2.0 * h[D]);
  const bool lc = a.lchol[s] != 0;
  double pv = 0.0;
  for (int g = 0; g < grp[s]; ++g) pv += partV[((size_t)g * a.S + s) * a.Nstar + i];
  const double mstar = gp_meanfun(a.meanfun, D, h + a.moff, a.Xs + i, (size_t)a.Nstar);
  const double fmu = mstar + partF[(size_t)s * a.Nstar + i];
  double fs2 = lc ? sf2 - pv : sf2 + pv;
  fs2 = fmax(fs2, 0.0);
  // noise at the test points (gplite_noisefun.m:176-207); the output-dependent term only with a non-empty ystar (:199)
  double sn2s = a.nf0 ? exp(2.0 * h[a.noff]) : 2.220446049250313e-16;
  if (a.nf1 == 1 && a.s2s) sn2s += a.s2s[i];
  else if (a.nf1 == 2 && a.s2s) sn2s += exp(h[a.noff + (a.nf0 ? 1 : 0)]) * a.s2s[i];
  if (a.nf2 == 1 && a.ys) {
    const int io = a.noff + (a.nf0 ? 1 : 0) + (a.nf1 == 2 ? 1 : 0);
    const double zz = fmax(0.0, h[io] - a.ys[i]);
    sn2s += exp(2.0 * h[io + 1]) * zz * zz;
  }
  a.fmu[i + (size_t)a.Nstar * s] = fmu;
  a.fs2[i + (size_t)a.Nstar * s] = fs2;
  a.ys2[i + (size_t)a.Nstar * s] = fs2 + sn2s * a.sn2_mult[s];
}

// The quadrature's closing step: F = m0 + nu + z * alpha (gplite_quad.m:77,82), nu = -1/2 sum_d (mu^2 + sigma^2 - 2 mu xm + xm^2) / omega^2
// for the negative quadratic mean (:80-81), nothing for the zero and constant means; varF = max(eps, nf_kk -/+ the block partials)
// (:101-106).  Written to fmu / fs2; k_pred_avg's fmu / fs2 columns are the averaging of :112-119.
__global__ void __launch_bounds__(256) k_quad_final(PredArgs a, const int* __restrict__ grp, const double* __restrict__ partV,
                                                    const double* __restrict__ partF) {
  const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= a.Nstar) return;
  const int D = a.D;
  const double* hm = a.hyp + (size_t)s * a.Nhyp + a.moff;
  double pv = 0.0;
  for (int g = 0; g < grp[s]; ++g) pv += partV[((size_t)g * a.S + s) * a.Nstar + i];
  double F = partF[(size_t)s * a.Nstar + i] + (a.meanfun > 0 ? hm[0] : 0.0);
  if (a.meanfun == 4) {
    double nu = 0.0;
    for (int d = 0; d < D; ++d) {
      const double m = a.Xs[i + (size_t)a.Nstar * d], xm = hm[1 + d], om = exp(hm[D + 1 + d]);
      nu += 1.0 / (om * om) * (m * m + a.qsig[d] * a.qsig[d] - 2.0 * m * xm + xm * xm);
    }
    F += -0.5 * nu;
  }
  const double nfkk = a.qnf[2 * s + 1];
  const double J = a.lchol[s] ? nfkk - pv : nfkk + pv;
  a.fmu[i + (size_t)a.Nstar * s] = F;
  a.fs2[i + (size_t)a.Nstar * s] = fmax(2.220446049250313e-16, J);
}

// gplite_pred.m:154-165 averaging over hyper-samples (in place into column 0 of the *_avg outputs)
__global__ void k_pred_avg(int Nstar, int S, const double* __restrict__ fmu, const double* __restrict__ fs2,
                           const double* __restrict__ ys2, double* __restrict__ out /* 4 x Nstar: ymu ys2 fmu fs2 */) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nstar) return;
  double fbar = 0.0, f2 = 0.0, y2 = 0.0;
  for (int s = 0; s < S; ++s) { fbar += fmu[i + (size_t)Nstar * s]; f2 += fs2[i + (size_t)Nstar * s]; y2 += ys2[i + (size_t)Nstar * s]; }
  fbar /= S;
  double vf = 0.0;
  for (int s = 0; s < S; ++s) { double d = fmu[i + (size_t)Nstar * s] - fbar; vf += d * d; }
  vf /= (S - 1);
  out[i] = fbar;                              // ymu = fmu without output warping
  out[i + (size_t)Nstar] = y2 / S + vf;       // ys2
  out[i + 2 * (size_t)Nstar] = fbar;          // fmu
  out[i + 3 * (size_t)Nstar] = f2 / S + vf;   // fs2
}

// Cross-covariance column for the rank-1 update (gplite_post.m:210-216): Ks[s][n] = k_s(X_n, x*),
// with sq_dist's two-argument centring for m = 1 test point.
__global__ void __launch_bounds__(256) k_gp_ks(int N, int D, int Nhyp, const double* __restrict__ X,
                                               const double* __restrict__ xstar, const double* __restrict__ hyp,
                                               const double* __restrict__ meanX, double* __restrict__ Ks) {
  const int s = blockIdx.y;
  const double* h = hyp + (size_t)s * Nhyp;
  __shared__ double ell[32], mu[32], xs[32];
  if (threadIdx.x < D) {
    const int d = threadIdx.x;
    ell[d] = exp(h[d]);
    const double n = (double)N, m = 1.0;
    mu[d] = (m / (n + m)) * (xstar[d] / ell[d]) + (n / (n + m)) * (meanX[d] / ell[d]);
    xs[d] = xstar[d] / ell[d] - mu[d];
  }
  __syncthreads();
  const double sf2 = exp(2.0 * h[D]);
  double bb = 0.0;
  for (int d = 0; d < D; ++d) bb = fma(xs[d], xs[d], bb);
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    double aa = 0.0, dot = 0.0;
    for (int d = 0; d < D; ++d) {
      double av = X[n + (size_t)N * d] / ell[d] - mu[d];
      aa = fma(av, av, aa);
      dot = fma(av, xs[d], dot);
    }
    Ks[(size_t)s * N + n] = sf2 * exp(-fmax(aa + (bb - 2.0 * dot), 0.0) / 2.0);
  }
}

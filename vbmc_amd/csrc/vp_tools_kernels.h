// The variational posterior in the caller's own parameter space, on the device: vbmc_pdf.m, vbmc_rnd.m, vbmc_moments.m:23-28 and
// vbmc_kldiv.m:70-88 with the variable transform of shared/warpvars_vbmc.m (types 0-3, scale row, rotation).
//   k_vp_pdf      one point per lane, the point in registers; the transform rows and the rotation in LDS; the mixture's components
//                 staged in LDS in chunks of 2048 / DT with an online log-sum-exp (one exponential per point and component)
//   k_vp_draw     row r -> sample pi(r) -> component -> mu + lambda (z sigma) -> inverse transform and clamp -> X, I
//   k_vp_moments  the same generation; per workgroup sum (x - c) and the upper triangle of sum (x - c)(x - c)' about a fixed centre c
//                 over tiles of 128 rows kept in LDS, every entry summed by one thread in row order
//   k_vp_kldiv    generation from one posterior, the densities of both at the original-space point, the rules of
//                 vbmc_kldiv.m:75-76 / :82-83, sum of log q_other - log q_own: lane in row order, wave shuffle, waves in order
//   k_vp_reduce   the per-workgroup partials added in index order (no fp64 atomics anywhere: DESIGN.md section 1)
// Randomness is an indexed block: sample i owns B[(D + 1) i ..]: slot 0 a uniform (catrnd of an unbalanced draw or of a remainder draw
// of the balanced split), slots 1 + d standard normals; generated from Philox counters (VPT_CTR, i, slot) keyed by the seed, or read
// from the caller's block.  The balanced split's randperm is a keyed bijection of [0, M) from integer operations alone (a six-round
// Feistel network on 2 hb bits with cycle walking), so that the host dump reproduces it.
// Kernels are templated on the padded dimension DT (4, 8, 12, 16, 24, 32): every per-dimension loop over registers is unrolled.
#pragma once
#include "common.h"
#include "dev_layout.h"
#include "device_math.h"   // vb_exp_tab
#include "parity_rng.h"    // srch_log, srch_normal, slice_uniform, slice_philox

#define VPT_T 128                 // threads per workgroup
#define VPT_TS (VPT_T + 1)        // stride of the per-thread stage columns (bank spread for the moments' row reads)
#define VPT_CHUNK 2048            // doubles of component means staged per chunk: 2048 / DT components
#define VPT_CTR 0xFFFFFFFDu
#define VPT_MAXBLK 512            // workgroups (= partials) of the reducing kernels: fixed, so that a result does not depend on the device
#define VPT_LOG_DENORM_MIN (-744.4400719213812)   // log(5e-324): the reference forms the density, which is zero below it
#define VPT_LOG_REALMIN (-708.3964185322641)      // log(realmin), vbmc_kldiv.m:70
#define VPT_NROWS 8               // transform rows: type, a, b, mu, delta, scale, lo, hi
enum { VPT_ROW_TYPE, VPT_ROW_A, VPT_ROW_B, VPT_ROW_MU, VPT_ROW_DELTA, VPT_ROW_SCALE, VPT_ROW_LO, VPT_ROW_HI };   // (the host's names for them)

struct VptPost {                  // one posterior; arrays padded to DT
  int D, K, fam, has_tr, has_rot, has_sc;   // fam 0: Gaussian, 1: multivariate t, 2: product of univariate t
  double lognf, dfa, ce, ljc;     // log normalisation, |df|, the t exponent, the constant part of the log-Jacobian
  const double *mus, *cst, *is2;  // K x DT mu / lambda; K log w - D log sigma; K 1 / sigma^2
  const double *mu, *sig;         // D x K, K (generation)
  const double *lam, *ilam;       // DT, DT
  const double* tr;               // VPT_NROWS x DT rows, then DT x DT rotation R(i, j) at [i DT + j]
};

// The packed block of one posterior, from the shape alone:  mus | cst | is2 | mu | sig | lam | ilam | tr   (tr with a trinfo only)
struct VptPackLayout {
  DevLayout L;
  DevWin<double> mus, cst, is2, mu, sig, lam, ilam, tr;
  VptPackLayout() {}
  VptPackLayout(int D, int DT, int K, bool has_tr) {
    mus = L.add<double>((size_t)K * DT); cst = L.add<double>(K); is2 = L.add<double>(K); mu = L.add<double>((size_t)D * K); sig = L.add<double>(K);
    lam = L.add<double>(DT); ilam = L.add<double>(DT); tr = L.add_if<double>(has_tr, (size_t)VPT_NROWS * DT + (size_t)DT * DT);
  }
  void bind(VptPost& P, const void* b) const {
    P.mus = mus.at(b); P.cst = cst.at(b); P.is2 = is2.at(b); P.mu = mu.at(b); P.sig = sig.at(b); P.lam = lam.at(b); P.ilam = ilam.at(b); P.tr = tr.at(b);
  }
};

struct VptGen {
  int N, M, M0, K, hb, balanced, parity, origflag;
  unsigned key[6];
  unsigned long long seed;
  const double* cdf;              // K: cumulative weights of catrnd
  const int* cum;                 // K + 1: cumulative counts of the balanced split
  const double* B;                // parity: (D + 1) M
};

template <int DT> struct VptTrS { double row[VPT_NROWS][DT]; double R[DT * DT]; };

// ---- the permutation
__host__ __device__ inline unsigned vpt_mix(unsigned r, unsigned k) {
  const unsigned long long p = (unsigned long long)0xD2511F53u * (unsigned long long)(r ^ k);
  unsigned h = (unsigned)(p >> 32) ^ (unsigned)p;
  h = (h ^ k) * 0xCD9E8D57u;
  return h ^ (h >> 15);
}
__host__ __device__ inline unsigned vpt_perm(unsigned r, unsigned M, int hb, const unsigned* key) {
  const unsigned mask = (1u << hb) - 1u;
  unsigned x = r;
  do {
    unsigned L = x >> hb, R = x & mask;
    for (int i = 0; i < 6; ++i) { const unsigned t = L ^ (vpt_mix(R, key[i]) & mask); L = R; R = t; }
    x = (L << hb) | R;
  } while (x >= M);
  return x;
}
__host__ __device__ inline void vpt_keys(unsigned long long seed, unsigned key[6]) {
  unsigned c0[4] = {0u, 0u, 0u, 4u}, c1[4] = {1u, 0u, 0u, 4u};
  slice_philox(c0, (unsigned)seed, (unsigned)(seed >> 32));
  slice_philox(c1, (unsigned)seed, (unsigned)(seed >> 32));
  key[0] = c0[0]; key[1] = c0[1]; key[2] = c0[2]; key[3] = c0[3]; key[4] = c1[0]; key[5] = c1[1];
}

// ---- logarithms from the search's own (a positive normal argument there)
__device__ __forceinline__ double vpt_log(double x) {
#pragma clang fp contract(off)
  if (!(x >= 0.0)) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (x == __builtin_inf()) return x;
  if (x < 2.2250738585072014e-308) return srch_log(x * 18014398509481984.0) - 37.42994775023705;   // 2^54, 54 ln 2
  return srch_log(x);
}
__device__ __forceinline__ double vpt_log1p(double v) {   // v >= 0: ln(w) v / (w - 1) carries the rounding of w = 1 + v away
#pragma clang fp contract(off)
  const double w = 1.0 + v;
  if (w == 1.0) return v;
  if (!(w < __builtin_inf())) return w;
  return srch_log(w) * v / (w - 1.0);
}

template <int DT>
__device__ __forceinline__ void vpt_stage_tr(const VptPost& P, VptTrS<DT>& S, int tid) {
  if (!P.has_tr) return;
  double* rows = &S.row[0][0];
  for (int e = tid; e < VPT_NROWS * DT; e += VPT_T) rows[e] = P.tr[e];
  if (P.has_rot)
    for (int e = tid; e < DT * DT; e += VPT_T) S.R[e] = P.tr[VPT_NROWS * DT + e];
}

// out_j = sum_i v_i R(i, j) (tr = false: y R) or sum_i v_i R(j, i) (tr = true: y R'), through this thread's stage column
template <int DT>
__device__ __forceinline__ void vpt_rot(double (&v)[DT], const double* R, bool tr, int D, double* col) {
#pragma unroll
  for (int i = 0; i < DT; ++i) col[i * VPT_TS] = v[i];
#pragma unroll
  for (int j = 0; j < DT; ++j) v[j] = 0.0;
  for (int i = 0; i < D; ++i) {
    const double vi = col[i * VPT_TS];
    if (tr) {
#pragma unroll
      for (int j = 0; j < DT; ++j) v[j] = fma(vi, R[j * DT + i], v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < DT; ++j) v[j] = fma(vi, R[i * DT + j], v[j]);
    }
  }
}

// warpvars_vbmc.m:85-110 (before the rotation and the scale)
template <int DT>
__device__ __forceinline__ void vpt_direct(double (&x)[DT], const VptTrS<DT>& S) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    const int t = (int)S.row[0][d];
    const double a = S.row[1][d], b = S.row[2][d], m = S.row[3][d], dl = S.row[4][d];
    if (t == 0) x[d] = (x[d] - m) / dl;
    else if (t == 1) x[d] = vpt_log(x[d] - a);
    else if (t == 2) x[d] = vpt_log(b - x[d]);
    else { const double z = (x[d] - a) / (b - a); x[d] = (vpt_log(z / (1.0 - z)) - m) / dl; }
  }
}
// warpvars_vbmc.m:296-320 and the clamp of :456-459
template <int DT>
__device__ __forceinline__ void vpt_inverse(double (&u)[DT], const VptTrS<DT>& S, const double* tab) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    const int t = (int)S.row[0][d];
    const double a = S.row[1][d], b = S.row[2][d], m = S.row[3][d], dl = S.row[4][d];
    double x;
    if (t == 0) x = u[d] * dl + m;
    else if (t == 1) x = vb_exp_tab<0>(fmin(u[d], 800.0), tab) + a;
    else if (t == 2) x = b - vb_exp_tab<0>(fmin(u[d], 800.0), tab);
    else { const double z = u[d] * dl + m; x = a + (b - a) * (1.0 / (1.0 + vb_exp_tab<0>(fmin(-z, 800.0), tab))); }
    u[d] = fmin(fmax(x, S.row[6][d]), S.row[7][d]);
  }
}
// the per-point part of warpvars_vbmc.m:484-503 (-z - 2 log1p(exp(-z)) is even in z: taken at |z|, which never overflows)
template <int DT>
__device__ __forceinline__ double vpt_logjac(const double (&u)[DT], const VptTrS<DT>& S, const double* tab) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    const int t = (int)S.row[0][d];
    if (t == 1 || t == 2) s = s + u[d];
    else if (t == 3) {
      const double az = fabs(u[d] * S.row[4][d] + S.row[3][d]);
      s = s + (-az - 2.0 * vpt_log1p(vb_exp_tab<0>(-az, tab)));
    }
  }
  return s;
}

// log of the mixture density at xs = y / lambda (vbmc_pdf.m:52-105 in the log domain), without the rule for an underflowing sum.
// Every thread of the workgroup calls it (the chunks are staged together).  GRAD: gn = d log p / d y (Gaussian family).
template <int DT, bool GRAD>
__device__ __forceinline__ double vpt_logmix(const double (&xs)[DT], const VptPost& P, double* s_mu, double* s_cst, double* s_is2, const double* tab, int tid,
                                             double (&gn)[DT]) {
  constexpr int KC = VPT_CHUNK / DT;
  double m = -__builtin_inf(), s = 0.0;
  double g[DT];
  if (GRAD) {
#pragma unroll
    for (int d = 0; d < DT; ++d) g[d] = 0.0;
  }
  for (int k0 = 0; k0 < P.K; k0 += KC) {
    const int kc = min(KC, P.K - k0);
    __syncthreads();
    for (int e = tid; e < kc * DT; e += VPT_T) s_mu[e] = P.mus[(size_t)k0 * DT + e];
    for (int e = tid; e < kc; e += VPT_T) { s_cst[e] = P.cst[k0 + e]; s_is2[e] = P.is2[k0 + e]; }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const double* mk = s_mu + k * DT;
      const double is2 = s_is2[k];
      double a;
      if (P.fam == 2) {
        double t = 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) { const double z = xs[d] - mk[d]; t += vpt_log1p(is2 * (z * z) / P.dfa); }
        a = s_cst[k] - P.ce * t;
      } else {
        double q = 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) { const double z = xs[d] - mk[d]; q = fma(z, z, q); }
        a = P.fam == 0 ? fma(-0.5 * is2, q, s_cst[k]) : s_cst[k] - P.ce * vpt_log1p(is2 * q / P.dfa);
      }
      // online log-sum-exp: the running maximum m and s = sum exp(a_k - m)
      const bool gt = a > m;
      const double e = vb_exp_tab<0>(-fabs(a - m), tab);
      s = gt ? fma(s, e, 1.0) : s + e;
      m = gt ? a : m;
      if (GRAD) {
        const double sc = gt ? e : 1.0, ck = (gt ? 1.0 : e) * is2;
#pragma unroll
        for (int d = 0; d < DT; ++d) g[d] = fma(g[d], sc, ck * (xs[d] - mk[d]));
      }
    }
  }
  if (GRAD) {
#pragma unroll
    for (int d = 0; d < DT; ++d) gn[d] = -(g[d] / s) * P.ilam[d];
  }
  if (!(s > 0.0)) return -__builtin_inf();
  return (m + srch_log(s)) + P.lognf;
}

// log vbmc_pdf(vp, x, origflag, 1, transflag, df) (vbmc_pdf.m:36-39, :52-105, :113-123); x is overwritten
template <int DT, bool GRAD>
__device__ __forceinline__ double vpt_eval(double (&x)[DT], const VptPost& P, const VptTrS<DT>& S, int origflag, int transflag, double* col, double* s_mu, double* s_cst,
                                           double* s_is2, const double* tab, int tid, double (&gn)[DT]) {
  double lj = 0.0;
  if (origflag && P.has_tr) {
    if (!transflag) {
      vpt_direct<DT>(x, S);
      lj = vpt_logjac<DT>(x, S, tab) + P.ljc;
      if (P.has_rot) vpt_rot<DT>(x, S.R, false, P.D, col);
      if (P.has_sc) {
#pragma unroll
        for (int d = 0; d < DT; ++d) x[d] = x[d] / S.row[5][d];
      }
    } else {
      double u[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) u[d] = P.has_sc ? x[d] * S.row[5][d] : x[d];
      if (P.has_rot) vpt_rot<DT>(u, S.R, true, P.D, col);
      lj = vpt_logjac<DT>(u, S, tab) + P.ljc;
    }
  }
#pragma unroll
  for (int d = 0; d < DT; ++d) x[d] = x[d] * P.ilam[d];
  double lt = vpt_logmix<DT, GRAD>(x, P, s_mu, s_cst, s_is2, tab, tid, gn);
  if (lt < VPT_LOG_DENORM_MIN) lt = -__builtin_inf();
  return lt - lj;
}

struct VptPdfArgs {
  VptPost P;
  int N, origflag, logflag, transflag;
  const double* X;     // N x D column-major
  double *y, *dy;      // N, N x D
};

template <int DT, bool GRAD>
__global__ void __launch_bounds__(VPT_T) k_vp_pdf(VptPdfArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[DT * VPT_TS];
  __shared__ double s_mu[VPT_CHUNK], s_cst[VPT_CHUNK / DT], s_is2[VPT_CHUNK / DT];
  __shared__ VptTrS<DT> S;
  const int tid = threadIdx.x, D = a.P.D, N = a.N;
  const long long r = (long long)blockIdx.x * VPT_T + tid;
  for (int j = tid; j < VB_EXP_TAB_N; j += VPT_T) tab[j] = c_exp2_tab[j];
  vpt_stage_tr<DT>(a.P, S, tid);
  __syncthreads();
  double x[DT], gn[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) x[d] = (d < D && r < N) ? a.X[(size_t)r + (size_t)N * d] : 0.0;
  double lo = vpt_eval<DT, GRAD>(x, a.P, S, a.origflag, a.transflag, stg + tid, s_mu, s_cst, s_is2, tab, tid, gn);
  if (r >= N) return;
  // x now holds the scaled transformed-space point.  A NaN among its D coordinates makes every term NaN, and a NaN term drops out
  // of the log-sum-exp through the table exponential's lower clamp: the result is NaN, as in the reference.  The padded registers do
  // not count: an infinite coordinate times the rotation's zero padding is NaN there, and the reference has no such column.
  bool isnan = false;
#pragma unroll
  for (int d = 0; d < DT; ++d) isnan = isnan || (d < D && x[d] != x[d]);
  if (isnan) lo = __builtin_nan("");
  const double pv = lo != lo ? lo : vb_exp_tab<0>(fmin(lo, 800.0), tab);   // (fmin drops a NaN: a point on or beyond a bound stays NaN)
  a.y[r] = a.logflag ? lo : pv;
  if (GRAD) {
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D) a.dy[(size_t)r + (size_t)N * d] = a.logflag ? gn[d] : gn[d] * pv;
  }
}

// ---- generation: row r -> sample pi(r) -> component -> the transformed-space sample into this thread's stage column
__device__ __forceinline__ int vpt_gen(const VptGen& G, const VptPost& P, const double* s_cdf, const int* s_cum, unsigned r, double* col) {
#pragma clang fp contract(off)
  const int D = P.D, K = G.K;
  const unsigned i = G.balanced ? vpt_perm(r, (unsigned)G.M, G.hb, G.key) : r;
  int lo = 0, hi = K;
  if (G.balanced && (int)i < G.M0) {                   // vbmc_rnd.m:59-64: the number of k with cum[k + 1] <= i
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_cum[mid + 1] <= (int)i) lo = mid + 1; else hi = mid; }
  } else {                                             // catrnd (:118-123): the number of k with cdf[k] < u cdf(end)
    const double u = G.parity ? G.B[(size_t)(D + 1) * i] : slice_uniform(G.seed, VPT_CTR, i, 0u);
    const double target = u * s_cdf[K - 1];
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_cdf[mid] < target) lo = mid + 1; else hi = mid; }
  }
  const int c = min(lo, K - 1);
  const double sg = P.sig[c];
  for (int d = 0; d < D; ++d) {
    const double z = G.parity ? G.B[(size_t)(1 + d) + (size_t)(D + 1) * i] : srch_normal(G.seed, VPT_CTR, i, (unsigned)d);
    col[d * VPT_TS] = P.mu[d + (size_t)D * c] + P.lam[d] * (z * sg);           // :84
  }
  return c;
}
// the staged sample into registers and, for origflag, back to the original space (warpvars_vbmc.m:284-288, :296-320, :456-459)
template <int DT>
__device__ __forceinline__ void vpt_finish(double (&x)[DT], const VptPost& P, const VptTrS<DT>& S, int origflag, double* col, const double* tab) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 0; d < DT; ++d) x[d] = d < P.D ? col[d * VPT_TS] : 0.0;
  if (!(origflag && P.has_tr)) return;
  if (P.has_sc) {
#pragma unroll
    for (int d = 0; d < DT; ++d) x[d] = x[d] * S.row[5][d];
  }
  if (P.has_rot) vpt_rot<DT>(x, S.R, true, P.D, col);
  vpt_inverse<DT>(x, S, tab);
}
__device__ __forceinline__ void vpt_stage_gen(const VptGen& G, double* s_cdf, int* s_cum, int tid) {
  for (int k = tid; k < G.K; k += VPT_T) s_cdf[k] = G.cdf[k];
  for (int k = tid; k <= G.K; k += VPT_T) s_cum[k] = G.cum[k];
}

struct VptDrawArgs {
  VptPost P;
  VptGen G;
  double* X;   // N x D column-major
  int* I;      // N, from 0
};

template <int DT>
__global__ void __launch_bounds__(VPT_T) k_vp_draw(VptDrawArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[DT * VPT_TS];
  __shared__ double s_cdf[VBMC_LIM_K];
  __shared__ int s_cum[VBMC_LIM_K + 1];
  __shared__ VptTrS<DT> S;
  const int tid = threadIdx.x, D = a.P.D, N = a.G.N;
  const long long r = (long long)blockIdx.x * VPT_T + tid;
  for (int j = tid; j < VB_EXP_TAB_N; j += VPT_T) tab[j] = c_exp2_tab[j];
  vpt_stage_tr<DT>(a.P, S, tid);
  vpt_stage_gen(a.G, s_cdf, s_cum, tid);
  __syncthreads();
  if (r >= N) return;
  const int c = vpt_gen(a.G, a.P, s_cdf, s_cum, (unsigned)r, stg + tid);
  double x[DT];
  vpt_finish<DT>(x, a.P, S, a.G.origflag, stg + tid, tab);
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (d < D) a.X[(size_t)r + (size_t)N * d] = x[d];
  if (a.I) a.I[r] = c;
}

// ---- moments: entry e < D is sum (x_e - c_e); the others the upper triangle (i <= j) column by column
struct VptMomArgs {
  VptPost P;
  VptGen G;
  const double* centre;            // DT
  const unsigned char *ei, *ej;    // nent: the rows of the tile an entry multiplies (row DT holds ones)
  int nent, ntile;
  double* partial;                 // gridDim.x x nent
};

// What k_vp_reduce folds, one block:  partial (the launches' per-workgroup sums) | out (their totals)
struct VptReduceBlock {
  DevLayout L;
  DevWin<double> partial, out;
  VptReduceBlock(size_t npartial, size_t nout) { partial = L.add<double>(npartial); out = L.add<double>(nout); }
};
// vbmc_vp_moments' entry table:  ei | ej, nent bytes each
struct VptMomEntries {
  DevLayout L;
  DevWin<unsigned char> ei, ej;
  explicit VptMomEntries(int nent) { ei = L.add<unsigned char>(nent); ej = L.add<unsigned char>(nent); }
  void bind(VptMomArgs& a, void* d) const { a.ei = ei.at(d); a.ej = ej.at(d); }
};

template <int DT>
__global__ void __launch_bounds__(VPT_T) k_vp_moments(VptMomArgs a) {
  constexpr int NE = DT + DT * (DT + 1) / 2, QM = (NE + VPT_T - 1) / VPT_T;
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[(DT + 1) * VPT_TS];
  __shared__ double s_cdf[VBMC_LIM_K];
  __shared__ int s_cum[VBMC_LIM_K + 1];
  __shared__ VptTrS<DT> S;
  const int tid = threadIdx.x, D = a.P.D, N = a.G.N;
  for (int j = tid; j < VB_EXP_TAB_N; j += VPT_T) tab[j] = c_exp2_tab[j];
  vpt_stage_tr<DT>(a.P, S, tid);
  vpt_stage_gen(a.G, s_cdf, s_cum, tid);
  stg[DT * VPT_TS + tid] = 1.0;
  int ri[QM], rj[QM];
  double acc[QM];
#pragma unroll
  for (int q = 0; q < QM; ++q) {
    const int e = tid + q * VPT_T;
    ri[q] = e < a.nent ? a.ei[e] * VPT_TS : 0;
    rj[q] = e < a.nent ? a.ej[e] * VPT_TS : 0;
    acc[q] = 0.0;
  }
  __syncthreads();
  for (int t = blockIdx.x; t < a.ntile; t += gridDim.x) {
    const long long r = (long long)t * VPT_T + tid;
    double x[DT];
    if (r < N) {
      vpt_gen(a.G, a.P, s_cdf, s_cum, (unsigned)r, stg + tid);
      vpt_finish<DT>(x, a.P, S, 1, stg + tid, tab);
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) stg[d * VPT_TS + tid] = (r < N && d < D) ? x[d] - a.centre[d] : 0.0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      double s = acc[q];
      for (int j = 0; j < VPT_T; ++j) s = fma(stg[ri[q] + j], stg[rj[q] + j], s);
      acc[q] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < QM; ++q) {
    const int e = tid + q * VPT_T;
    if (e < a.nent) a.partial[(size_t)blockIdx.x * a.nent + e] = acc[q];
  }
}

// The family's one workgroup sum of T threads, the same value in every thread: lane sums by wave shuffle, the waves in index order
template <int T>
__device__ __forceinline__ double vpt_block_sum(double v, double* s_w, int tid) {
#pragma clang fp contract(off)
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  __syncthreads();
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < T / 64; ++w) s = s + s_w[w];
  return s;
}

// out[e] = sum_b partial[b nent + e], b in index order
__global__ void __launch_bounds__(VPT_T) k_vp_reduce(const double* partial, int nb, int nent, double* out) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * VPT_T + threadIdx.x;
  if (e >= nent) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + partial[(size_t)b * nent + e];
  out[e] = s;
}

// ---- one direction of vbmc_kldiv.m:72-77: generate from Pg, sum of log q_other - log q_own
struct VptKlArgs {
  VptPost Pg, Po;
  VptGen G;
  int ntile;
  double* xx;          // N x D or null
  double* partial;     // gridDim.x
};

template <int DT>
__global__ void __launch_bounds__(VPT_T) k_vp_kldiv(VptKlArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[DT * VPT_TS];
  __shared__ double s_mu[VPT_CHUNK], s_cst[VPT_CHUNK / DT], s_is2[VPT_CHUNK / DT];
  __shared__ double s_cdf[VBMC_LIM_K];
  __shared__ int s_cum[VBMC_LIM_K + 1];
  __shared__ double s_w[VPT_T / 64];
  __shared__ VptTrS<DT> Sg, So;
  const int tid = threadIdx.x, D = a.Pg.D, N = a.G.N;
  for (int j = tid; j < VB_EXP_TAB_N; j += VPT_T) tab[j] = c_exp2_tab[j];
  vpt_stage_tr<DT>(a.Pg, Sg, tid);
  vpt_stage_tr<DT>(a.Po, So, tid);
  vpt_stage_gen(a.G, s_cdf, s_cum, tid);
  __syncthreads();
  double acc = 0.0;
  for (int t = blockIdx.x; t < a.ntile; t += gridDim.x) {
    const long long r = (long long)t * VPT_T + tid;
    double x[DT], u[DT], gn[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) x[d] = 0.0;
    if (r < N) {
      vpt_gen(a.G, a.Pg, s_cdf, s_cum, (unsigned)r, stg + tid);
      vpt_finish<DT>(x, a.Pg, Sg, 1, stg + tid, tab);
      if (a.xx) {
#pragma unroll
        for (int d = 0; d < DT; ++d)
          if (d < D) a.xx[(size_t)r + (size_t)N * d] = x[d];
      }
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) u[d] = x[d];
    const double lg = vpt_eval<DT, false>(u, a.Pg, Sg, 1, 0, stg + tid, s_mu, s_cst, s_is2, tab, tid, gn);
#pragma unroll
    for (int d = 0; d < DT; ++d) u[d] = x[d];
    const double lo = vpt_eval<DT, false>(u, a.Po, So, 1, 0, stg + tid, s_mu, s_cst, s_is2, tab, tid, gn);
    if (r < N) {
#pragma clang fp contract(off)
      // the reference forms the densities, replaces the zero and the non-finite ones, and takes the logarithms (:73-77)
      const double qg = vb_exp_tab<0>(fmin(lg, 800.0), tab), qo = vb_exp_tab<0>(fmin(lo, 800.0), tab);
      const bool bg = !(qg > 0.0) || !(qg < __builtin_inf()), bo = !(qo > 0.0) || !(qo < __builtin_inf());
      const double tg = bg ? 0.0 : vpt_log(qg), to = bo ? VPT_LOG_REALMIN : vpt_log(qo);
      acc = acc + (to - tg);
    }
  }
  acc = vpt_block_sum<VPT_T>(acc, s_w, tid);
  if (tid == 0) a.partial[blockIdx.x] = acc;
}

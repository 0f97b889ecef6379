// The data of a corner plot on the device: utils/cornerplot.m:113-156 (a histogram per dimension, utils/kde2d.m per pair of dimensions)
// and the order statistics of utils/quantile1.m:37-72 over one sample matrix X (Ns x D column-major), vbmc_vp_corner's kernels.
// n = res (16, 32 or 64) is kde2d's grid; pair pp of (d1 < d2) in cornerplot.m:154-155's order.
//   k_corner_range   one workgroup per column: min, max, a finiteness flag -> MIN, MAX (the caller's bounds if given, :93-96, :116)
//   k_corner_index   grid (slices of Ns, D): per sample the bin of ndhist (kde2d.m:88, :188-189) as one byte, 0 = outside, and the
//                    nbins histogram of the column between its bounds (LDS counts, then integer atomics on global memory)
//   k_corner_pairs   grid (slices of Ns, P): ndhist's accumarray (:193) from two bytes per sample, n^2 int32 counts in LDS, the
//                    non-zero ones added to global memory by integer atomics (integer addition is order-free)
//   k_corner_kde     one workgroup per pair, the n x n tile in LDS: dct2d (:142-161) as the direct sums it stands for, the bracket of
//                    root() (:196-212) and k_mtv_root's safeguarded secant on t - evolve(t) (:110-136, the 18 psi nodes of func's
//                    recursion memoised by s), t_x, t_y (:96-98), a_t (:100), idct2d (:163-176) into kde2d's transposed layout
//                    with the scale of :103 and the clamp of :104
//   k_corner_select  one workgroup per (rank, column): the exact order statistic by a radix descent, eight bits at a time, on
//                    order-preserving 64-bit keys with an LDS digit histogram (no sort of the matrix; ties come out as sort's)
// Every floating-point sum has a fixed order (thread in index order, vpt_block_sum); the counts are integers.  Nothing depends on
// the grid.
#pragma once
#include "mtv_kernels.h"   // MTV_T, MTV_EPS, MTV_PI2, mtv_locate, mtv_finite; vpt_block_sum, vpt_log, vb_exp_tab behind it

#define CORNER_T MTV_T            // threads per workgroup
#define CORNER_MAXBINS 1024       // nbins
#define CORNER_MAXQ 16            // probabilities; two ranks each

struct CornerCol {                // one column (written by k_corner_range)
  double MIN, MAX;                // the bounds of the histogram and of kde2d's grid
  int bad, nonfinite;             // no bounds given and the range is zero; an entry is not finite
};

struct CornerRangeArgs {
  int Ns;
  const double* x;                // Ns x D column-major; one workgroup per column
  const double* bounds;           // 2 x D, or null: the column's min and max
  CornerCol* col;                 // D
};

__global__ void __launch_bounds__(CORNER_T) k_corner_range(CornerRangeArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_lo[CORNER_T / 64], s_hi[CORNER_T / 64];
  __shared__ int s_nf[CORNER_T / 64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const double* x = a.x + (size_t)a.Ns * c;
  double lo = __builtin_inf(), hi = -__builtin_inf();
  int nf = 0;
  for (int i = tid; i < a.Ns; i += CORNER_T) {
    const double v = x[i];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
    nf |= mtv_finite(v) ? 0 : 1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
    nf |= __shfl_xor(nf, o, 64);
  }
  if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; s_nf[tid >> 6] = nf; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < CORNER_T / 64; ++w) { lo = fmin(lo, s_lo[w]); hi = fmax(hi, s_hi[w]); nf |= s_nf[w]; }
  CornerCol q;
  q.MIN = a.bounds ? a.bounds[2 * c] : lo;
  q.MAX = a.bounds ? a.bounds[2 * c + 1] : hi;
  const double R = q.MAX - q.MIN;
  q.bad = !(R > 0.0 && R < __builtin_inf()) ? 1 : 0;
  q.nonfinite = nf;
  a.col[c] = q;
}

struct CornerIndexArgs {
  int Ns, n, nbins;
  const double* x;                // Ns x D
  const CornerCol* col;           // D
  unsigned char* idx;             // Ns x D: ndhist's bin 1 .. n, 0 = dropped
  int* hist;                      // nbins x D, zeroed
};

__global__ void __launch_bounds__(CORNER_T) k_corner_index(CornerIndexArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_h[CORNER_MAXBINS];
  const int tid = threadIdx.x, c = blockIdx.y;
  const CornerCol q = a.col[c];
  const double scaling = q.MAX - q.MIN, w = scaling / (double)a.nbins, rn = (double)a.n;
  const double* x = a.x + (size_t)a.Ns * c;
  unsigned char* idx = a.idx + (size_t)a.Ns * c;
  for (int j = tid; j < a.nbins; j += CORNER_T) s_h[j] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * CORNER_T + tid; i < a.Ns; i += (long long)gridDim.x * CORNER_T) {
    const double v = x[i];
    const double t = (v - q.MIN) / scaling;                                               // kde2d.m:88
    int b = 0;
    if (t >= 0.0 && t <= 1.0) b = t == 1.0 ? a.n : (int)(t * rn) + 1;                     // :188-189 (k / n is exact: histc)
    idx[i] = (unsigned char)b;
    if (!q.bad && v >= q.MIN && v <= q.MAX) atomicAdd(&s_h[mtv_locate(v, q.MIN, w, a.nbins - 1)], 1);
  }
  __syncthreads();
  for (int j = tid; j < a.nbins; j += CORNER_T)
    if (s_h[j] != 0) atomicAdd(a.hist + (size_t)c * a.nbins + j, s_h[j]);
}

struct CornerPairsArgs {
  int Ns, n;
  const unsigned char* idx;       // Ns x D
  const int* pairs;               // P x 2: d1, d2
  int* counts2;                   // n x n x P, zeroed: (bin of d1) + n (bin of d2)
};

__global__ void __launch_bounds__(CORNER_T) k_corner_pairs(CornerPairsArgs a) {
  __shared__ int s_h[64 * 64];
  const int tid = threadIdx.x, pp = blockIdx.y, n2 = a.n * a.n;
  const unsigned char* i1 = a.idx + (size_t)a.Ns * a.pairs[2 * pp];
  const unsigned char* i2 = a.idx + (size_t)a.Ns * a.pairs[2 * pp + 1];
  for (int j = tid; j < n2; j += CORNER_T) s_h[j] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * CORNER_T + tid; i < a.Ns; i += (long long)gridDim.x * CORNER_T) {
    const int b1 = i1[i], b2 = i2[i];
    if (b1 > 0 && b2 > 0) atomicAdd(&s_h[(b1 - 1) + a.n * (b2 - 1)], 1);                  // all(bins > 0, 2), kde2d.m:193
  }
  __syncthreads();
  int* out = a.counts2 + (size_t)pp * n2;
  for (int j = tid; j < n2; j += CORNER_T)
    if (s_h[j] != 0) atomicAdd(out + j, s_h[j]);
}

// ---- kde2d on one pair
struct CornerKdeArgs {
  int n, Ns;
  const CornerCol* col;           // D
  const int* pairs;               // P x 2
  const int* counts2;             // n x n x P
  const double* tab;              // n + 1: cos(pi m / (2 n)), the quarter wave
  double* density;                // n x n x P: row the d2 mesh, column the d1 mesh (kde2d.m:103)
  double* txy;                    // 2 x P: t_x, t_y
  double* tstar;                  // P
  int* status;                    // P: 0 a root, 1 no bracket below 0.1 (the reference's fminbnd branch), 2 a bad column
  double pi2l[6];                 // pi^(2 l), l = 0 .. 5
  double kk[5];                   // K(s) (kde2d.m:138-140), s = 0 .. 4
  double cst[5];                  // (1 + 1 / 2^(l + 1)) / 3 (:120), l = 0 .. 4
  double pi;
};

// cos(pi m / (2 n)) from the quarter wave, n a power of two
__device__ __forceinline__ double corner_cos(unsigned m, unsigned n, const double* s_tab) {
  unsigned r = m & (4u * n - 1u);
  if (r > 2u * n) r = 4u * n - r;                                                         // cos(2 pi - t) = cos t
  const bool neg = r > n;                                                                 // cos(pi - t) = -cos t
  if (neg) r = 2u * n - r;
  const double cv = s_tab[r];
  return neg ? -cv : cv;
}

// One direction of dct2d / idct2d over the tile s_a (element (i, j) at i + N j), in place, every thread's N^2 / T outputs held in
// registers across the barrier.  ALONG 0: over the row index, 1: over the column index.  Forward: out_k = f_k sum_j in_j c(k, j),
// f_0 = 1, f_k = 2; inverse: out_j = sum_k in_k c(k, j); c(k, j) = cos(pi k (2 j + 1) / (2 N)).  The sum runs in index order.
template <int N, int ALONG, bool INV>
__device__ __forceinline__ void corner_dct_pass(double* s_a, const double* s_tab, int tid, double (&acc)[(N * N + CORNER_T - 1) / CORNER_T]) {
  constexpr int Q = (N * N + CORNER_T - 1) / CORNER_T;
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0;
  for (int s = 0; s < N; ++s) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = tid + q * CORNER_T;
      if (N * N >= CORNER_T || e < N * N) {
        const int i = e % N, j = e / N, o = ALONG == 0 ? i : j;
        const unsigned m = INV ? (unsigned)s * (2u * (unsigned)o + 1u) : (unsigned)o * (2u * (unsigned)s + 1u);
        const double v = ALONG == 0 ? s_a[s + N * j] : s_a[i + N * s];
        acc[q] = fma(v, corner_cos(m, N, s_tab), acc[q]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int e = tid + q * CORNER_T;
    if (N * N >= CORNER_T || e < N * N) {
      const int o = ALONG == 0 ? e % N : e / N;
      s_a[e] = (!INV && o > 0) ? 2.0 * acc[q] : acc[q];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ double corner_pow(double x, double y, const double* tab) {
#pragma clang fp contract(off)
  if (!(x >= 0.0)) return __builtin_nan("");                                              // (the reference's power is complex there)
  return mtv_powexp(x, y, tab);
}

// I^s, I = k^2, s = 0 .. 5 (0^0 = 1)
__device__ __forceinline__ double corner_ipow(double I, int s) {
#pragma clang fp contract(off)
  const double I2 = I * I;
  return s == 0 ? 1.0 : s == 1 ? I : s == 2 ? I2 : s == 3 ? I2 * I : s == 4 ? I2 * I2 : (I2 * I2) * I;
}

// one workgroup's LDS: the tile, the quarter wave, psi's two weight rows, vpt_block_sum's row, the values of two levels of func's
// recursion, the constants (pi^(2 l) at [l], K(s) at [6 + s], the const of kde2d.m:120 at [11 + l]) and the exponential's table
struct CornerLds {
  double *a, *cosq, *wx, *wy, *w, *f, *k;
  const double* tab;
};

// psi([s1, s2], Time) (kde2d.m:129-136) over A2 = a .^ 2, a the tile
template <int N>
__device__ __forceinline__ double corner_psi(int s1, int s2, double Time, const CornerLds& S, int tid) {
#pragma clang fp contract(off)
  __syncthreads();
  if (tid < N) {
    const double I = (double)tid * (double)tid, arg = (-I * MTV_PI2) * Time;
    const double e = arg != arg ? arg : vb_exp_tab<0>(arg, S.tab);                        // (the table exponential's clamp would drop a NaN)
    const double w = tid == 0 ? e : e * 0.5;                                              // :132
    S.wx[tid] = w * corner_ipow(I, s1);                                                   // :133
    S.wy[tid] = w * corner_ipow(I, s2);                                                   // :134
  }
  __syncthreads();
  double s = 0.0;
  for (int e = tid; e < N * N; e += CORNER_T) {
    const double v = S.a[e];
    s = s + (S.wy[e % N] * (v * v)) * S.wx[e / N];                                        // wy * A2 * wx'
  }
  s = vpt_block_sum<CORNER_T>(s, S.w, tid);
  const double sg = ((s1 + s2) & 1) ? -1.0 : 1.0;
  return (sg * s) * S.k[s1 + s2];                                                         // :135
}

// func's recursion (kde2d.m:117-127) from the six leaves [i, 5 - i] at t down to [0, 2], [1, 1], [2, 0]: f2[i] = func([i, 2 - i], t).
// 18 psi nodes: a node's value depends on (s, t) alone, and every sum keeps func's order.  The values of a level live in LDS
// (S.f: the level above, S.f + 6: the level being made), so that the loops stay loops.
template <int N>
__device__ __forceinline__ void corner_func2(double t, double Nd, const CornerLds& S, int tid, double (&f2)[3]) {
#pragma clang fp contract(off)
#pragma nounroll
  for (int i = 0; i <= 5; ++i) {
    const double v = corner_psi<N>(i, 5 - i, t, S, tid);                                  // :124
    if (tid == 0) S.f[i] = v;
  }
#pragma nounroll
  for (int L = 4; L >= 2; --L) {
#pragma nounroll
    for (int i = 0; i <= L; ++i) {
      __syncthreads();
      const double Sum = S.f[i + 1] + S.f[i];                                             // func([s1 + 1, s2]) + func([s1, s2 + 1]), :120
      const double time = corner_pow(-2.0 * S.k[11 + L] * S.k[6 + i] * S.k[6 + L - i] / Nd / Sum, 1.0 / (2.0 + (double)L), S.tab);   // :121
      const double v = corner_psi<N>(i, L - i, time, S, tid);                             // :122
      if (tid == 0) S.f[6 + i] = v;
    }
    __syncthreads();
    if (tid <= L) S.f[tid] = S.f[6 + tid];
  }
  __syncthreads();
  f2[0] = S.f[0]; f2[1] = S.f[1]; f2[2] = S.f[2];
}

// t - evolve(t) (kde2d.m:95, :110-115)
template <int N>
__device__ __forceinline__ double corner_objective(double t, double Nd, double pi, const CornerLds& S, int tid) {
#pragma clang fp contract(off)
  double f2[3];
  corner_func2<N>(t, Nd, S, tid, f2);
  const double Sum = f2[0] + f2[2] + 2.0 * f2[1];                                         // :112
  const double time = corner_pow(2.0 * pi * Nd * Sum, -1.0 / 3.0, S.tab);                 // :113
  return t - (t - time) / time;                                                           // :114, :95
}

template <int N>
__device__ __forceinline__ void corner_kde_body(const CornerKdeArgs& A, const CornerLds& S) {
#pragma clang fp contract(off)
  constexpr int Q = (N * N + CORNER_T - 1) / CORNER_T;
  const int tid = threadIdx.x, pp = blockIdx.x;
  double *s_a = S.a, *s_tab = S.cosq, *s_wx = S.wx, *s_wy = S.wy;
  const double* tab = S.tab;
  const CornerCol q1 = A.col[A.pairs[2 * pp]], q2 = A.col[A.pairs[2 * pp + 1]];
  double* dens = A.density + (size_t)pp * N * N;
  const double nan = __builtin_nan("");
  auto fail = [&](int status) {
    for (int e = tid; e < N * N; e += CORNER_T) dens[e] = nan;
    if (tid == 0) { A.txy[2 * pp] = nan; A.txy[2 * pp + 1] = nan; A.tstar[pp] = nan; A.status[pp] = status; }
  };
  if (q1.bad || q2.bad) { fail(2); return; }
  const double Nd = (double)A.Ns;                                                         // kde2d.m:79: every row, the dropped ones included
  const int* cnt = A.counts2 + (size_t)pp * N * N;
  for (int e = tid; e < N * N; e += CORNER_T) s_a[e] = (double)cnt[e] / Nd;               // :193
  for (int j = tid; j <= N; j += CORNER_T) s_tab[j] = A.tab[j];
  if (tid < 6) S.k[tid] = A.pi2l[tid];
  if (tid < 5) { S.k[6 + tid] = A.kk[tid]; S.k[11 + tid] = A.cst[tid]; }
  __syncthreads();
  double acc[Q];
  corner_dct_pass<N, 0, false>(s_a, s_tab, tid, acc);                                     // :152
  corner_dct_pass<N, 1, false>(s_a, s_tab, tid, acc);

  // root() (:196-212); every thread carries the same scalars
  const double Nc = fmin(fmax(Nd, 50.0), 1050.0);                                         // :198
  double tol = 1e-12 + 0.01 * (Nc - 50.0) / 1000.0;                                       // :199
  auto F = [&](double t) { return corner_objective<N>(t, Nd, A.pi, S, tid); };
  double lo = 0.0, flo = F(0.0), hi = tol, fhi = 0.0;
  bool found = false;
  for (int it = 0; it < 64; ++it) {                                                       // :201-211
    fhi = F(tol);
    hi = tol;
    if (mtv_finite(flo) && mtv_finite(fhi) && ((flo <= 0.0 && fhi >= 0.0) || (flo >= 0.0 && fhi <= 0.0))) { found = true; break; }
    tol = fmin(tol * 2.0, 0.1);
    if (tol == 0.1) break;
  }
  if (!found) { fail(1); return; }
  double t;
  if (flo == 0.0) t = lo;
  else if (fhi == 0.0) t = hi;
  else {
    // k_mtv_root's iteration: a secant step from the bracket's ends (Illinois weights), kept inside the bracket, followed by a
    // bisection whenever the step has not halved the bracket; ends when the bracket is a few ulps wide or f == 0
    int side = 0;
    bool done = false;
    auto take = [&](double x) {
      const double fx = F(x);
      if (fx == 0.0) { lo = hi = x; done = true; }
      else if (!mtv_finite(fx)) done = true;
      else if ((fx < 0.0) == (flo < 0.0)) { lo = x; flo = fx; if (side == -1) fhi = 0.5 * fhi; side = -1; }
      else { hi = x; fhi = fx; if (side == 1) flo = 0.5 * flo; side = 1; }
    };
    for (int it = 0; it < 200 && !done; ++it) {
      const double wdt = hi - lo;
      if (wdt <= 4.0 * MTV_EPS * fmax(fabs(hi), 2.2250738585072014e-308)) break;
      double x = (lo * fhi - hi * flo) / (fhi - flo);
      if (!(x > lo && x < hi)) x = lo + 0.5 * wdt;
      if (!(x > lo && x < hi)) break;
      take(x);
      if (done || hi - lo <= 0.5 * wdt) continue;
      x = lo + 0.5 * (hi - lo);
      if (x > lo && x < hi) take(x);
    }
    t = lo + 0.5 * (hi - lo);
  }
  double p[3];                                                                            // p_02, p_11, p_20 (:96)
  corner_func2<N>(t, Nd, S, tid, p);
  const double p02 = p[0], p11 = p[1], p20 = p[2];
  const double den = p11 + sqrt(p20 * p02);
  const double p02q = corner_pow(p02, 0.75, tab), p20q = corner_pow(p20, 0.75, tab);
  const double t_y = corner_pow(p02q / (4.0 * A.pi * Nd * p20q * den), 1.0 / 3.0, tab);   // :97
  const double t_x = corner_pow(p20q / (4.0 * A.pi * Nd * p02q * den), 1.0 / 3.0, tab);   // :98
  __syncthreads();
  if (tid < N) {
    const double I = (double)tid * (double)tid;
    s_wx[tid] = vb_exp_tab<0>(((-I * MTV_PI2) * t_x) / 2.0, tab);
    s_wy[tid] = vb_exp_tab<0>(((-I * MTV_PI2) * t_y) / 2.0, tab);
  }
  __syncthreads();
  for (int e = tid; e < N * N; e += CORNER_T) s_a[e] = (s_wx[e % N] * s_wy[e / N]) * s_a[e];   // :100
  __syncthreads();
  corner_dct_pass<N, 0, true>(s_a, s_tab, tid, acc);                                      // :169
  corner_dct_pass<N, 1, true>(s_a, s_tab, tid, acc);
  const double scale = (double)(N * N) / ((q1.MAX - q1.MIN) * (q2.MAX - q2.MIN)), inv = 1.0 / (double)(N * N);
  for (int e = tid; e < N * N; e += CORNER_T) {
    double v = (s_a[e] * inv) * scale;                                                    // ifft's 1 / n in each direction; :103
    if (v < 0.0) v = MTV_EPS;                                                             // :104
    dens[(e / N) + N * (e % N)] = v;                                                      // idct2d's one transpose
  }
  if (tid == 0) { A.txy[2 * pp] = t_x; A.txy[2 * pp + 1] = t_y; A.tstar[pp] = t; A.status[pp] = 0; }
}

__global__ void __launch_bounds__(CORNER_T) k_corner_kde(CornerKdeArgs A) {
  __shared__ double s_a[64 * 64];
  __shared__ double s_tab[64 + 1], s_wx[64], s_wy[64];
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double s_w[CORNER_T / 64], s_f[12], s_k[16];
  for (int j = threadIdx.x; j < VB_EXP_TAB_N; j += CORNER_T) tab[j] = c_exp2_tab[j];
  const CornerLds S{s_a, s_tab, s_wx, s_wy, s_w, s_f, s_k, tab};
  if (A.n == 64) corner_kde_body<64>(A, S);
  else if (A.n == 32) corner_kde_body<32>(A, S);
  else corner_kde_body<16>(A, S);
}

// ---- order statistics
struct CornerSelectArgs {
  int Ns, nrank;
  const double* x;                // Ns x D
  const int* rank;                // nrank: from 0, < Ns
  double* out;                    // nrank x D
};

// the order of the doubles as an order of unsigned integers (a NaN with a clear sign bit above +Inf, as sort places it)
__device__ __forceinline__ unsigned long long corner_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(CORNER_T) k_corner_select(CornerSelectArgs a) {
  __shared__ int s_h[256];
  __shared__ int s_digit, s_rank;
  const int tid = threadIdx.x, c = blockIdx.y;
  const double* x = a.x + (size_t)a.Ns * c;
  unsigned long long prefix = 0ull;
  int r = a.rank[blockIdx.x];
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_h[tid] = 0;
    __syncthreads();
    for (int i = tid; i < a.Ns; i += CORNER_T) {
      const unsigned long long k = corner_key(x[i]);
      if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_h[(int)((k >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int d = 0, below = 0;
      while (d < 255 && below + s_h[d] <= r) { below += s_h[d]; ++d; }
      s_digit = d;
      s_rank = r - below;
    }
    __syncthreads();
    prefix |= (unsigned long long)s_digit << shift;
    r = s_rank;
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long u = (prefix >> 63) ? (prefix & 0x7FFFFFFFFFFFFFFFull) : ~prefix;
    a.out[(size_t)c * a.nrank + blockIdx.x] = __longlong_as_double((long long)u);
  }
}

// The marginal total variation between posteriors on the device: vbmc_mtv.m:24-79 with shared/kde1d.m:35-140 (Botev's diffusion
// estimator) and shared/qtrapz.m, for vbmc_vp_mtv's two posteriors and vbmc_vp_diagnostics' R runs alike.  The draws are k_vp_draw's
// (vp_tools_kernels.h), one run at a time; a column is one (run, dimension) pair, col = i D + d.
//   k_mtv_mesh      one run's D columns, one workgroup each: min and max of the draws, the counts on the two clamp ends -> MIN, MAX, N
//                   (vbmc_mtv.m:55-63, kde1d.m:46)
//   k_mtv_bin       one run's D columns: histc on the uniform mesh (kde1d.m:48), integer atomics on global memory (integer addition
//                   is order-free)
//   k_mtv_init      initial_data = counts / N, divided by its sum (kde1d.m:48)
//   k_mtv_dct       dct1d (kde1d.m:113-122) resp. idct1d (:94-110) as the direct sums they stand for,
//                     a_0 = sum_j x_j, a_k = 2 sum_j x_j cos(pi k (2 j + 1) / (2 n)),   out_j = sum_k a_k cos(pi k (2 j + 1) / (2 n)),
//                   one output per thread, the cosine from a host-made quarter-wave table of n + 1 doubles in LDS
//   k_mtv_root      one workgroup per column: the bracket of root() (kde1d.m:124-140) and a bisection-safeguarded secant iteration on
//                   fixed_point (:79-89) down to a bracket a few ulps wide; then a_t = a exp(-k^2 pi^2 t / 2) (:55)
//   k_mtv_integral  vbmc_mtv.m:73-78 for every pair of runs and dimension in one launch: both not-a-knot splines at nquad points of
//                   each of the three segments, the trapezoid sums as MTV_NBLK per-workgroup partials per entry that k_vp_reduce
//                   adds in index order
// Every floating-point sum has a fixed order (thread in index order, vpt_block_sum); nothing depends on the grid, on R or on which
// other runs are in the call.
#pragma once
#include "vp_tools_kernels.h"

#define MTV_T 256                 // threads per workgroup
#define MTV_NBLK 128              // workgroups (= partials) per dimension of the integral: fixed, so that a result does not depend on the device
#define MTV_EPS 2.220446049250313e-16
#define MTV_PI2 9.869604401089358 // pi^2

struct MtvCol {                   // one column's mesh (written by k_mtv_mesh)
  double MIN, MAX, N;             // N: the unique count of kde1d.m:46 by the clamp-end rule
  int bad, pad;                   // the draws' range is zero or not finite: NaN for this dimension
};

struct MtvMeshArgs {
  int Ns;
  const double* x;                // Ns x D column-major: one run's draws; one workgroup per column
  const double* ends;             // D x 4: lb_orig, ub_orig, the clamp ends lb + eps(lb), ub - eps(ub) (+-Inf: none)
  MtvCol* col;                    // D
  long long* nuniq;               // D
};

__global__ void __launch_bounds__(MTV_T) k_mtv_mesh(MtvMeshArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_lo[MTV_T / 64], s_hi[MTV_T / 64];
  __shared__ int s_cl[MTV_T / 64], s_ch[MTV_T / 64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const double* x = a.x + (size_t)a.Ns * c;
  const double lb = a.ends[4 * c], ub = a.ends[4 * c + 1], el = a.ends[4 * c + 2], eh = a.ends[4 * c + 3];
  double lo = __builtin_inf(), hi = -__builtin_inf();
  int cl = 0, ch = 0;
  for (int i = tid; i < a.Ns; i += MTV_T) {
    const double v = x[i];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
    cl += v == el ? 1 : 0;
    ch += v == eh ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
    cl += __shfl_xor(cl, o, 64);
    ch += __shfl_xor(ch, o, 64);
  }
  if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; s_cl[tid >> 6] = cl; s_ch[tid >> 6] = ch; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < MTV_T / 64; ++w) { lo = fmin(lo, s_lo[w]); hi = fmax(hi, s_hi[w]); cl += s_cl[w]; ch += s_ch[w]; }
  const double range = hi - lo;
  const double MIN = fmax(lo - range / 10.0, lb), MAX = fmin(hi + range / 10.0, ub);   // vbmc_mtv.m:55-63
  const double R = MAX - MIN;
  const bool el_on = el > -__builtin_inf() && el < __builtin_inf(), eh_on = eh > -__builtin_inf() && eh < __builtin_inf();
  const long long nu = (long long)a.Ns - (el_on && cl > 1 ? cl - 1 : 0) - (eh_on && ch > 1 ? ch - 1 : 0);
  MtvCol q;
  q.MIN = MIN; q.MAX = MAX; q.N = (double)nu; q.pad = 0;
  q.bad = !(range > 0.0 && range < __builtin_inf() && R > 0.0 && R < __builtin_inf()) ? 1 : 0;
  a.col[c] = q;
  a.nuniq[c] = nu;
}

// the largest k <= last with MIN + k dx <= x (histc; what lies at or beyond the last edge goes to `last`)
__device__ __forceinline__ int mtv_locate(double x, double MIN, double dx, int last) {
#pragma clang fp contract(off)
  const double q = (x - MIN) / dx;
  int k = q >= (double)last ? last : (q > 0.0 ? (int)q : 0);
  while (k > 0 && MIN + (double)k * dx > x) --k;
  while (k < last && MIN + (double)(k + 1) * dx <= x) ++k;
  return k;
}

struct MtvBinArgs {
  int Ns, n;
  const double* x;                // Ns x D column-major: one run's draws; blockIdx.y is the column
  const MtvCol* col;              // D
  int* counts;                    // D x n, zeroed
};

__global__ void __launch_bounds__(MTV_T) k_mtv_bin(MtvBinArgs a) {
#pragma clang fp contract(off)
  const int c = blockIdx.y;
  const MtvCol q = a.col[c];
  if (q.bad) return;
  const double dx = (q.MAX - q.MIN) / (double)(a.n - 1);                                // kde1d.m:46
  const double* x = a.x + (size_t)a.Ns * c;
  int* cnt = a.counts + (size_t)c * a.n;
  for (long long i = (long long)blockIdx.x * MTV_T + threadIdx.x; i < a.Ns; i += (long long)gridDim.x * MTV_T) {
    const double v = x[i];
    if (v != v) continue;                                                                 // (histc does not count a NaN)
    atomicAdd(cnt + mtv_locate(v, q.MIN, dx, a.n - 1), 1);
  }
}

struct MtvInitArgs {
  int n;
  const MtvCol* col;
  const int* counts;
  double* x;                      // 2 D x n
};

__global__ void __launch_bounds__(MTV_T) k_mtv_init(MtvInitArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_w[MTV_T / 64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const MtvCol q = a.col[c];
  const int* cnt = a.counts + (size_t)c * a.n;
  double* x = a.x + (size_t)c * a.n;
  if (q.bad) {
    for (int j = tid; j < a.n; j += MTV_T) x[j] = 0.0;
    return;
  }
  double s = 0.0;
  for (int j = tid; j < a.n; j += MTV_T) s = s + (double)cnt[j] / q.N;
  s = vpt_block_sum<MTV_T>(s, s_w, tid);
  for (int j = tid; j < a.n; j += MTV_T) x[j] = ((double)cnt[j] / q.N) / s;               // kde1d.m:48
}

// out_o = f_o sum_i in_i cos(pi m / (2 n)), m = o (2 i + 1) (forward, f_0 = 1, f_o = 2) or i (2 o + 1) (inverse, f = 1).
// m mod 4 n folds into the quarter wave: tab[m] = cos(pi m / (2 n)), m = 0 .. n.  Four partial sums over i mod 4, each in index order.
struct MtvDctArgs {
  int n, inverse;
  const double* tab;              // n + 1
  const double* in;               // 2 D x n
  double* out;                    // 2 D x n
  double* a2;                     // forward: 2 D x n, (a_k / 2)^2 (kde1d.m:51); or null
};

__global__ void __launch_bounds__(MTV_T) k_mtv_dct(MtvDctArgs a) {
  extern __shared__ double s_tab[];
  const int tid = threadIdx.x, n = a.n, c = blockIdx.y;
  for (int j = tid; j <= n; j += MTV_T) s_tab[j] = a.tab[j];
  __syncthreads();
  const unsigned o = blockIdx.x * MTV_T + tid, n2 = 2u * (unsigned)n, m4 = 4u * (unsigned)n - 1u;
  if (o >= (unsigned)n) return;
  const double* in = a.in + (size_t)c * n;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const unsigned step = a.inverse ? 2u * o + 1u : 2u * o;      // m(i + 1) - m(i)
  unsigned m = a.inverse ? 0u : o;
  for (int i = 0; i < n; i += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unsigned r = m & m4;
      if (r > n2) r = 2u * n2 - r;                             // cos(2 pi - t) = cos t
      const bool neg = r > (unsigned)n;                        // cos(pi - t) = -cos t
      if (neg) r = n2 - r;
      const double cv = s_tab[r];
      acc[u] = fma(in[i + u], neg ? -cv : cv, acc[u]);
      m += step;
    }
  }
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (!a.inverse && o > 0) s = 2.0 * s;
  a.out[(size_t)c * n + o] = s;
  if (a.a2) { const double h = 0.5 * s; a.a2[(size_t)c * n + o] = h * h; }
}

// ---- fixed_point (kde1d.m:79-89)
struct MtvRootArgs {
  int n, D;
  const MtvCol* col;
  const double* a;                // 2 D x n: the cosine coefficients
  const double* a2;               // 2 D x n
  double* at;                     // 2 D x n: a exp(-k^2 pi^2 t / 2)
  double* tstar;                  // 2 D
  int* status;                    // 2 D: 0 a root, 1 no bracket below 0.1 (the reference's fminbnd branch), 2 a bad column
  double pi2l[8];                 // pi^(2 l), l = 2 .. 7
  double ck[8];                   // 2 const K0 of step s = 2 .. 6 (:84)
  double sqrtpi;
};

// sum_k k^(2 l) a2_k exp(-k^2 pi^2 t), k = 1 .. n - 1
template <int L>
__device__ __forceinline__ double mtv_gamma_sum(const double* a2, int n, double t, const double* tab, double* s_w, int tid) {
#pragma clang fp contract(off)
  double s = 0.0;
  const double c = -MTV_PI2 * t;
  for (int k = 1 + tid; k < n; k += MTV_T) {
    const double I = (double)k * (double)k, I2 = I * I, I3 = I2 * I;
    const double p = L == 2 ? I2 : L == 3 ? I3 : L == 4 ? I2 * I2 : L == 5 ? I3 * I2 : L == 6 ? I3 * I3 : (I3 * I3) * I;
    const double arg = I * c;
    const double e = arg != arg ? arg : vb_exp_tab<0>(arg, tab);   // (the table exponential's clamp would drop a NaN)
    s = s + (p * a2[k]) * e;
  }
  return vpt_block_sum<MTV_T>(s, s_w, tid);
}

__device__ __forceinline__ double mtv_powexp(double x, double y, const double* tab) {
#pragma clang fp contract(off)
  if (x != x) return x;
  if (!(x > 0.0)) return y > 0.0 ? 0.0 : __builtin_inf();
  if (x == __builtin_inf()) return y > 0.0 ? x : 0.0;
  return vb_exp_tab<0>(fmin(y * vpt_log(x), 800.0), tab);
}

__device__ __forceinline__ double mtv_fixed_point(double t, const MtvRootArgs& A, const double* a2, double N, const double* tab, double* s_w, int tid) {
#pragma clang fp contract(off)
  const int n = A.n;
  double f = 2.0 * A.pi2l[7] * mtv_gamma_sum<7>(a2, n, t, tab, s_w, tid);
#define MTV_STEP(S)                                                                      \
  {                                                                                      \
    const double time = mtv_powexp(A.ck[S] / N / f, 2.0 / (3.0 + 2.0 * S), tab);         \
    f = 2.0 * A.pi2l[S] * mtv_gamma_sum<S>(a2, n, time, tab, s_w, tid);                  \
  }
  MTV_STEP(6) MTV_STEP(5) MTV_STEP(4) MTV_STEP(3) MTV_STEP(2)
#undef MTV_STEP
  return t - mtv_powexp(2.0 * N * A.sqrtpi * f, -2.0 / 5.0, tab);
}

__device__ __forceinline__ bool mtv_finite(double v) { return v > -__builtin_inf() && v < __builtin_inf(); }

__global__ void __launch_bounds__(MTV_T) k_mtv_root(MtvRootArgs A) {
#pragma clang fp contract(off)
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double s_w[MTV_T / 64];
  const int tid = threadIdx.x, c = blockIdx.x, n = A.n;
  for (int j = tid; j < VB_EXP_TAB_N; j += MTV_T) tab[j] = c_exp2_tab[j];
  __syncthreads();
  const MtvCol q = A.col[c];
  const double* a2 = A.a2 + (size_t)c * n;
  double* at = A.at + (size_t)c * n;
  if (q.bad) {
    for (int k = tid; k < n; k += MTV_T) at[k] = 0.0;
    if (tid == 0) { A.tstar[c] = __builtin_nan(""); A.status[c] = 2; }
    return;
  }
  // every thread carries the same scalars: the sums are broadcast by vpt_block_sum
  const double Nc = fmin(fmax(q.N, 50.0), 1050.0);                                        // kde1d.m:126
  double tol = 1e-12 + 0.01 * (Nc - 50.0) / 1000.0;                                       // :127
  const double f0 = mtv_fixed_point(0.0, A, a2, q.N, tab, s_w, tid);
  double lo = 0.0, flo = f0, hi = tol, fhi = 0.0;
  bool found = false;
  for (int it = 0; it < 64; ++it) {                                                       // :129-139
    fhi = mtv_fixed_point(tol, A, a2, q.N, tab, s_w, tid);
    hi = tol;
    if (mtv_finite(flo) && mtv_finite(fhi) && ((flo <= 0.0 && fhi >= 0.0) || (flo >= 0.0 && fhi <= 0.0))) { found = true; break; }
    tol = fmin(tol * 2.0, 0.1);
    if (tol == 0.1) break;
  }
  if (!found) {
    for (int k = tid; k < n; k += MTV_T) at[k] = 0.0;
    if (tid == 0) { A.tstar[c] = __builtin_nan(""); A.status[c] = 1; }
    return;
  }
  double t;
  if (flo == 0.0) t = lo;
  else if (fhi == 0.0) t = hi;
  else {
    // a secant step from the bracket's ends (Illinois weights), kept inside the bracket, followed by a bisection whenever the step
    // has not halved the bracket.  Ends when the bracket is a few ulps wide or f == 0.
    int side = 0;
    bool done = false;
    auto take = [&](double x) {
      const double fx = mtv_fixed_point(x, A, a2, q.N, tab, s_w, tid);
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
  const double h = -0.5 * MTV_PI2 * t;
  const double* a = A.a + (size_t)c * n;
  for (int k = tid; k < n; k += MTV_T) at[k] = a[k] * vb_exp_tab<0>(((double)k * (double)k) * h, tab);   // kde1d.m:55
  if (tid == 0) { A.tstar[c] = t; A.status[c] = 0; }
}

// ---- the integral (vbmc_mtv.m:73-78)
struct MtvIntArgs {
  int n, D, nquad, ntile, npair;
  const int* pairs;               // npair x 2: the runs i < j of a pair; its columns are i D + d and j D + d
  const double* geo;              // npair x D x 4: bb, the four mesh ends sorted (vbmc_mtv.m:74)
  const double* msh;              // R D x 4: MIN, dx, the last mesh point, bad
  const double* yy;               // R D x n: the normalised densities
  const double* mm;               // R D x n: the splines' second derivatives times dx^2 / 6
  double* partial;                // MTV_NBLK x 3 D npair
};

// The KDE pipeline's work block, from the shape alone (nC = R D x n mesh values):  initial data | a | a2 | a_t | the inverse transform
struct MtvWork {
  DevLayout w;
  DevWin<double> x, a, a2, at, raw;
  MtvWork() = default;
  explicit MtvWork(size_t nC) { x = w.add<double>(nC); a = w.add<double>(nC); a2 = w.add<double>(nC); at = w.add<double>(nC); raw = w.add<double>(nC); }
};
// The two input blocks of k_mtv_integral:  s: yy | mm (nC each)        g: msh (4 R D) | geo (4 D npair)
struct MtvIntBlocks {
  DevLayout s, g;
  DevWin<double> yy, mm, msh, geo;
  MtvIntBlocks(size_t nC, size_t nmsh, size_t ngeo) { yy = s.add<double>(nC); mm = s.add<double>(nC); msh = g.add<double>(nmsh); geo = g.add<double>(ngeo); }
  void bind(MtvIntArgs& ia, void* ds, void* dg) const { ia.yy = yy.at(ds); ia.mm = mm.at(ds); ia.msh = msh.at(dg); ia.geo = geo.at(dg); }
};

// the not-a-knot spline of column c at x; 0 outside its mesh (interp1(..., 'spline', 0))
__device__ __forceinline__ double mtv_spline(const MtvIntArgs& a, int c, double x) {
#pragma clang fp contract(off)
  const double MIN = a.msh[4 * c], dx = a.msh[4 * c + 1], last = a.msh[4 * c + 2];
  if (!(x >= MIN && x <= last)) return 0.0;
  const int i = mtv_locate(x, MIN, dx, a.n - 2);
  const double* y = a.yy + (size_t)c * a.n;
  const double* m = a.mm + (size_t)c * a.n;
  const double s = (x - (MIN + (double)i * dx)) / dx, r = 1.0 - s;
  return (y[i] * r + y[i + 1] * s) + (m[i] * (r * r * r - r) + m[i + 1] * (s * s * s - s));
}

// grid (partial, dimension, pair)
__global__ void __launch_bounds__(MTV_T) k_mtv_integral(MtvIntArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_w[MTV_T / 64];
  const int tid = threadIdx.x, d = blockIdx.y, p = blockIdx.z;
  const int c1 = a.pairs[2 * p] * a.D + d, c2 = a.pairs[2 * p + 1] * a.D + d;
  const size_t e = (size_t)p * a.D + d, nent = 3 * (size_t)a.D * a.npair;
  const bool bad = a.msh[4 * c1 + 3] != 0.0 || a.msh[4 * c2 + 3] != 0.0;
  for (int j = 0; j < 3; ++j) {
    const double b0 = a.geo[4 * e + j], b1 = a.geo[4 * e + j + 1];
    const double step = (b1 - b0) / (double)(a.nquad - 1);                               // linspace
    double acc = 0.0;
    if (!bad && b1 > b0) {
      for (int t = blockIdx.x; t < a.ntile; t += gridDim.x) {
        const int i = t * MTV_T + tid;
        if (i < a.nquad) {
          const double x = i == a.nquad - 1 ? b1 : b0 + (double)i * step;
          const double v = fabs(mtv_spline(a, c1, x) - mtv_spline(a, c2, x));
          acc = acc + ((i == 0 || i == a.nquad - 1) ? 0.5 * v : v);                      // qtrapz
        }
      }
    }
    acc = vpt_block_sum<MTV_T>(acc, s_w, tid);
    if (tid == 0) a.partial[(size_t)blockIdx.x * nent + 3 * e + j] = acc;
  }
}

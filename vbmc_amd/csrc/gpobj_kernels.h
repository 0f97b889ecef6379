// The device half of the GP objective that the slice sampler (slice_kernels.h) and the train optimiser (trainopt_kernels.h) share:
// what turns one candidate hyper-parameter vector into the inputs of the batched gplite_nlZ path (k_gp_scale .. k_nlz_final,
// gp_factor.h: gp_launch_*), and the noise inflation between two tries of a checked factorisation.  Both callers promise their
// results bit for bit (W-invariance, parity with the NumPy restatements), so there is one copy of this arithmetic.
#pragma once
#include "common.h"
#include "dev_layout.h"
#include "device_math.h"

// What gpobj_emit reads and writes.  SliceKernelArgs and ToptArgs derive from it.
struct GpObjArgs {
  int N, Nhyp, Ncov, Nnoise, nf0, nf1, nf2, has_prior;
  const double *y, *s2;                       // N (s2 may be null)
  const double *pmu, *psig, *pdf, *pc;        // Nhyp: hyper-prior location, scale, degrees of freedom, normalising term
  const int* ptype;                           // Nhyp: 0 flat, 1 Gaussian, 2 Student-t
  double *hyp, *sn2, *scal, *lp;              // B x Nhyp, B x N, B x 4, B
  double *dsn2, *dlp;                         // GRAD only: B x Nnoise x N, B x Nhyp
};

// The windows of both callers' input block that GpObjArgs points into: the head X | y | s2 (s2 keeps its N doubles when the caller
// has none, and is then null) and the hyper-prior's rows pmu | psig | pdf | pc.
struct GpObjHead {
  DevWin<double> X, y, s2;
  void add(DevLayout& L, int N, int D, bool has_s2) { X = L.add<double>((size_t)N * D); y = L.add<double>(N); s2 = L.add<double>(N, has_s2); }
  void pack(void* img, const double* X_, const double* y_, const double* s2_) const { X.put(img, X_); y.put(img, y_); s2.put(img, s2_); }
  double* bind(GpObjArgs& a, void* base) const { a.y = y.at(base); a.s2 = s2.at(base); return X.at(base); }   // returns X
};
struct GpObjPrior {
  DevWin<double> pmu, psig, pdf, pc;
  void add(DevLayout& L, int Nhyp) { pmu = L.add<double>(Nhyp); psig = L.add<double>(Nhyp); pdf = L.add<double>(Nhyp); pc = L.add<double>(Nhyp); }
  void pack(void* img, const double* mu, const double* sig, const double* df, const double* c) const { pmu.put(img, mu); psig.put(img, sig); pdf.put(img, df); pc.put(img, c); }
  void bind(GpObjArgs& a, void* base) const { a.pmu = pmu.at(base); a.psig = psig.at(base); a.pdf = pdf.at(base); a.pc = pc.at(base); }
};

// MATLAB's eps(x) for a finite x
__device__ __forceinline__ double matlab_eps(double x) {
  const double ax = fabs(x);
  if (ax < 2.2250738585072014e-308) return 4.9406564584124654e-324;
  int e;
  (void)frexp(ax, &e);
  return ldexp(1.0, e - 53);
}

// One workgroup of 256 threads writes everything the batched gplite_nlZ path needs for candidate b, whose hyper-parameters hv(i)
// returns: the hyper-parameter row, the noise vector and its Cholesky branch (gplite_core.m:33-40,67, gplite_noisefun.m:176-210)
// and the hyper-prior (gplite_hypprior.m:17-65); with GRAD the noise derivatives and the prior's gradient too.
template <bool GRAD, class HV>
__device__ __forceinline__ void gpobj_emit(const GpObjArgs& a, int b, HV hv) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N;
  double* h = a.hyp + (size_t)b * a.Nhyp;
  for (int i = tid; i < a.Nhyp; i += 256) h[i] = hv(i);
  // noise variance per training point and its derivatives
  int idx = a.Ncov, i0 = -1, i1 = -1, i2 = -1;
  double base = 2.220446049250313e-16, c1 = 0.0, ythr = 0.0, w2 = 0.0;
  if (a.nf0 == 1) { base = exp(2.0 * hv(idx)); i0 = idx - a.Ncov; idx++; }
  if (a.nf1 == 2) { c1 = exp(hv(idx)); i1 = idx - a.Ncov; idx++; }
  if (a.nf2 == 1) { ythr = hv(idx); w2 = exp(2.0 * hv(idx + 1)); i2 = idx - a.Ncov; }
  double* ds = GRAD ? a.dsn2 + (size_t)b * a.Nnoise * N : nullptr;
  double mn = __builtin_inf();
  for (int n = tid; n < N; n += 256) {
    double v = base;
    if (a.nf1 == 1 && a.s2) v += a.s2[n];
    else if (a.nf1 == 2 && a.s2) v += c1 * a.s2[n];
    if (GRAD && i0 >= 0) ds[(size_t)i0 * N + n] = 2.0 * base;
    if (GRAD && i1 >= 0) ds[(size_t)i1 * N + n] = a.s2 ? c1 * a.s2[n] : 0.0;
    if (i2 >= 0) {
      const double df = ythr - a.y[n], zz = fmax(0.0, df);
      v += w2 * zz * zz;
      if (GRAD) {
        ds[(size_t)i2 * N + n] = zz > 0.0 ? 2.0 * w2 * df : 0.0;
        ds[(size_t)(i2 + 1) * N + n] = 2.0 * w2 * zz * zz;
      }
    }
    a.sn2[(size_t)b * N + n] = v;
    mn = fmin(mn, v);
  }
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64));
  if (lane == 0) red[wave] = mn;
  __syncthreads();
  if (tid == 0) {
    mn = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    const bool lch = mn >= 1e-6;
    double* sc = a.scal + (size_t)b * 4;
    sc[0] = lch ? mn : 1.0;      // sn2div
    sc[1] = 1.0;                 // sn2_mult
    sc[2] = lch ? 1.0 : 0.0;
    sc[3] = lch ? mn : 1.0;      // sl = sn2div * sn2_mult
  }
  if (wave == 0) {
    double t = 0.0;
    for (int i = lane; i < a.Nhyp; i += 64) {
      const int ty = a.has_prior ? a.ptype[i] : 0;
      double dl = 0.0;
      if (ty != 0) {
        const double z = (hv(i) - a.pmu[i]) / a.psig[i], z2 = z * z;
        if (ty == 1) { t += -0.5 * (a.pc[i] + z2); dl = -z / a.psig[i]; }
        else {
          const double nu = a.pdf[i];
          t += a.pc[i] - 0.5 * (nu + 1.0) * log1p(z2 / nu);
          dl = -(nu + 1.0) / nu / (1.0 + z2 / nu) * z / a.psig[i];
        }
      }
      if (GRAD) a.dlp[(size_t)b * a.Nhyp + i] = dl;
    }
    t = wave_sum(t);
    if (lane == 0) a.lp[b] = t;
  }
}

// The x10 noise inflation of a checked round (gplite_core.m:77-80,91-94) between two tries of the factorisation: a matrix that
// came out positive definite is switched off, one that failed gets ten times the jitter.
__global__ void k_gpobj_retry(int B, const int* __restrict__ pf, double* __restrict__ scal, unsigned char* __restrict__ act) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= B || !act[w]) return;
  if (pf[w] > 0) {
    const double m = scal[w * 4 + 1] * 10.0;
    scal[w * 4 + 1] = m;
    scal[w * 4 + 3] = scal[w * 4 + 2] != 0.0 ? scal[w * 4 + 0] * m : 1.0;
  } else act[w] = 0;
}

// The library's reproducible generator, host and device: Philox4x32-10 counters keyed by the seed -> uniforms, permutation words and
// (through Wichura's AS 241) normals, and the one-rounding-per-operation proposal step of the slice samplers.  The *_rng_dump entry
// points reproduce on the host, bit for bit, what the kernels draw.  (Not device_math.h's philox4x32 / vb_normal4*: that is the
// seven-round generator of the entropy kernels.)
// The slice_ / srch_ prefixes are historical: the functions were written for the slice sampler and the acquisition search and are now
// used by every sampler of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

// ---- the library's own uniforms: Philox4x32-10 keyed by the seed, counter (sweep, idd, slot, stream); 52 bits -> (0, 1).
// Integer arithmetic and exactly representable fp64 steps: the host (vbmc_slice_rng_dump) and the device compute the same bits.
__host__ __device__ inline void slice_philox(unsigned c[4], unsigned k0, unsigned k1) {
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__host__ __device__ inline double slice_uniform(unsigned long long seed, unsigned sweep, unsigned idd, unsigned slot) {
  unsigned c[4] = {sweep, idd, slot, 0u};
  slice_philox(c, (unsigned)seed, (unsigned)(seed >> 32));
  const double v = (double)(c[0] >> 6) * 67108864.0 + (double)(c[1] >> 6);   // < 2^52: exact
  return (v + 0.5) * 2.220446049250313e-16;                                  // (v + 1/2) 2^-52
}
__host__ __device__ inline unsigned slice_perm_word(unsigned long long seed, unsigned sweep, unsigned j) {
  unsigned c[4] = {sweep, j, 0u, 1u};
  slice_philox(c, (unsigned)seed, (unsigned)(seed >> 32));
  return c[0];
}

// xprime(dd) = rand()*(x_r(dd) - x_l(dd)) + x_l(dd)   (:286), every operation rounded on its own.  The compiler contracts a multiply
// and an add into an fma unless told otherwise -- inside the __d*_rn intrinsics too, whose bodies are plain operators compiled with the
// default setting, so they are no protection: the chain's own arithmetic is written with plain operators in a scope with contraction off --
// this recursion, the interval placement, the burn-in sums whose variance of a FIXED coordinate is zero or a rounding error of either
// sign (:347-349) --, so that it is MATLAB's arithmetic operation for operation.
__device__ __forceinline__ double slice_prop(double u, double xl, double xr) {
#pragma clang fp contract(off)
  return u * (xr - xl) + xl;
}

// ---- the library's own normals: Philox4x32-10 keyed by the seed, counter (generation, point, d); 52 bits -> u in (0, 1) -> the
// inverse normal CDF by Wichura's AS 241 (PPND16).  Only +, -, *, /, sqrt and integer operations, each rounded on its own (contraction
// off) -- the logarithm of the tail branch included (srch_log) --, so that the host (vbmc_acq_search_rng_dump) and the device compute
// the same bits.
__host__ __device__ inline double srch_log(double x) {   // ln x for a positive normal x, |error| ~ 1e-16 relative
#pragma clang fp contract(off)
  unsigned long long b;
  memcpy(&b, &x, 8);
  int e = (int)((b >> 52) & 0x7ff) - 1023;
  b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m;
  memcpy(&m, &b, 8);                                     // [1, 2)
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }   // [sqrt(1/2), sqrt(2)]
  const double t = (m - 1.0) / (m + 1.0), t2 = t * t;    // ln m = 2 atanh t, t^2 <= 0.0295
  double s = 1.0 / 27.0;
  s = s * t2 + 1.0 / 25.0; s = s * t2 + 1.0 / 23.0; s = s * t2 + 1.0 / 21.0; s = s * t2 + 1.0 / 19.0; s = s * t2 + 1.0 / 17.0;
  s = s * t2 + 1.0 / 15.0; s = s * t2 + 1.0 / 13.0; s = s * t2 + 1.0 / 11.0; s = s * t2 + 1.0 / 9.0; s = s * t2 + 1.0 / 7.0;
  s = s * t2 + 1.0 / 5.0; s = s * t2 + 1.0 / 3.0; s = s * t2 + 1.0;
  return (double)e * 0.6931471805599453 + 2.0 * t * s;
}
__host__ __device__ inline double srch_ndtri(double p) {
#pragma clang fp contract(off)
  const double q = p - 0.5;
  if (q >= -0.425 && q <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                           1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                          5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0;
    return num / den;
  }
  double r = q < 0.0 ? p : 1.0 - p;
  r = sqrt(-srch_log(r));
  double x;
  if (r <= 5.0) {
    r = r - 1.6;
    const double num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                          3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
    const double den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                          6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0;
    x = num / den;
  } else {
    r = r - 5.0;
    const double num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                          2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
    const double den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                          1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0;
    x = num / den;
  }
  return q < 0.0 ? -x : x;
}
__host__ __device__ inline double srch_normal(unsigned long long seed, unsigned gen, unsigned point, unsigned d) {
  unsigned c[4] = {gen, point, d, 2u};
  slice_philox(c, (unsigned)seed, (unsigned)(seed >> 32));
  const double v = (double)(c[0] >> 6) * 67108864.0 + (double)(c[1] >> 6);   // < 2^52: exact
  return srch_ndtri((v + 0.5) * 2.220446049250313e-16);
}

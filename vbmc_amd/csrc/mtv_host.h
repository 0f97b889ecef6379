// Host pieces of the marginal total variation that vbmc_vp_mtv (abi_vp_mtv.hip) and vbmc_vp_diagnostics (abi_vp_diag.hip) share: the
// constants of fixed_point (kde1d.m:84), the quarter-wave cosine table, and the O(n) tail of a column between the inverse transform and
// the integral (kde1d.m:58-62, vbmc_mtv.m:68,71) with its not-a-knot spline system (a serial recurrence).
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "mtv_kernels.h"

namespace {
// m = M dx^2 / 6 of the not-a-knot cubic spline through y on a uniform mesh (M the second derivatives):
// m_{i-1} + 4 m_i + m_{i+1} = y_{i-1} - 2 y_i + y_{i+1}; m_0 - 2 m_1 + m_2 = 0 and its mirror image give 6 m_1 = r_1, 6 m_{n-2} = r_{n-2}
void mtv_spline_host(const double* y, int n, double* m, std::vector<double>& cp) {
  auto r = [&](int i) { return (y[i - 1] - 2.0 * y[i]) + y[i + 1]; };
  cp.assign(n, 0.0);
  m[1] = r(1) / 6.0;
  m[n - 2] = r(n - 2) / 6.0;
  cp[2] = 0.25;
  m[2] = (r(2) - m[1]) / 4.0;
  for (int i = 3; i <= n - 3; ++i) {
    const double den = 4.0 - cp[i - 1];
    cp[i] = 1.0 / den;
    m[i] = ((i == n - 3 ? r(i) - m[n - 2] : r(i)) - m[i - 1]) / den;
  }
  for (int i = n - 4; i >= 2; --i) m[i] = m[i] - cp[i] * m[i + 1];
  m[0] = 2.0 * m[1] - m[2];
  m[n - 1] = 2.0 * m[n - 2] - m[n - 3];
}

// tab[m] = cos(pi m / (2 n)), m = 0 .. n: the quarter wave k_mtv_dct folds every cosine into
void mtv_cos_table(int n, std::vector<double>& htab) {
  htab.resize((size_t)n + 1);
  for (int m = 0; m <= n; ++m) htab[m] = (double)cosl(3.14159265358979323846264338327950288L * (long double)m / (long double)(2 * n));
  htab[n] = 0.0;
}

// the constants of fixed_point (kde1d.m:84)
void mtv_root_consts(MtvRootArgs& a) {
  const double pi = 3.14159265358979323846;
  for (int l = 2; l <= 7; ++l) a.pi2l[l] = std::pow(pi, 2.0 * l);
  for (int s = 2; s <= 6; ++s) {
    double prod = 1.0;
    for (int j = 1; j <= 2 * s - 1; j += 2) prod *= j;
    const double K0 = prod / std::sqrt(2.0 * pi), cst = (1.0 + std::pow(0.5, s + 0.5)) / 3.0;
    a.ck[s] = 2.0 * cst * K0;
  }
  a.sqrtpi = std::sqrt(pi);
}

// kde1d.m:58, :62 and vbmc_mtv.m:68, :71 on one column of the inverse transform (y, overwritten by the normalised density), then its
// spline (m) and its mesh row msh[4]: MIN, dx, the last mesh point, bad
void mtv_finish_column(const MtvCol& q, int n, double* y, double* m, double* msh, std::vector<double>& cp) {
  if (q.bad) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int j = 0; j < n; ++j) { y[j] = nan; m[j] = 0.0; }
    msh[0] = q.MIN; msh[1] = 0.0; msh[2] = q.MIN; msh[3] = 1.0;
    return;
  }
  const double R = q.MAX - q.MIN, dx = R / (double)(n - 1);
  double sum = 0.0;
  for (int j = 0; j < n; ++j) {
    double v = y[j] / R;                                                               // kde1d.m:58
    if (v < 0.0) v = MTV_EPS;                                                           // :62
    y[j] = v;
    sum += v;
  }
  const double qt = sum - 0.5 * (y[0] + y[n - 1]), h = (q.MIN + dx) - q.MIN;            // qtrapz; xmesh(2) - xmesh(1)
  const double nrm = qt * h;
  for (int j = 0; j < n; ++j) y[j] = y[j] / nrm;                                        // vbmc_mtv.m:68, :71
  mtv_spline_host(y, n, m, cp);
  msh[0] = q.MIN; msh[1] = dx; msh[2] = q.MIN + (double)(n - 1) * dx; msh[3] = 0.0;
}
}  // namespace

// Host side of vbmc_vp_corner (abi_vp_mtv.hip): the argument checks, the constants of kde2d's func / psi / K (utils/kde2d.m:117-140),
// the ranks and the interpolation of utils/quantile1.m:37-72, and CornerPipeline: the one sequence of allocations, launches, copies
// back and host tails that takes a sample matrix on the device to the histograms, the pair densities and the quantiles.  It is a
// pipeline of its own, not an MtvPipeline: the columns share nothing with kde1d's beyond the cosine table and the root iteration
// (no unique count, no mesh extension, no spline, no integral), and the unit of work is a pair, not a column.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "corner_kernels.h"
#include "mtv_host.h"       // mtv_cos_table
#include "vp_tools_host.h"  // VptPack, VptGenHost, VPT_FOR_DT, VPT_MAXN

namespace {
// the constants of func, psi and K
void corner_kde_consts(CornerKdeArgs& a) {
  const double pi = 3.14159265358979323846;
  a.pi = pi;
  for (int l = 0; l <= 5; ++l) a.pi2l[l] = std::pow(pi, 2.0 * l);                         // kde2d.m:135
  for (int s = 0; s <= 4; ++s) {
    double prod = 1.0;
    for (int j = 1; j <= 2 * s - 1; j += 2) prod *= j;
    a.kk[s] = ((s & 1) ? -1.0 : 1.0) * prod / std::sqrt(2.0 * pi);                        // :139
    a.cst[s] = (1.0 + 1.0 / std::pow(2.0, s + 1.0)) / 3.0;                                // :120
  }
}

// quantile1.m:37-72 for the probabilities p on a column of n values none of which is NaN: the 1-based ranks k and kp1 and the ratio r
struct CornerQuant {
  int nq = 0;
  bool median = false;                   // isequal(p, 0.5): the branch of :40-45
  std::vector<long long> k, kp1;
  std::vector<double> r;
  std::vector<int> ranks;                // the distinct ranks, from 0
  std::vector<int> ik, ikp1;             // where each probability's two ranks are in `ranks`

  int slot(long long rank1) {
    const int r0 = (int)(rank1 - 1);
    for (size_t i = 0; i < ranks.size(); ++i)
      if (ranks[i] == r0) return (int)i;
    ranks.push_back(r0);
    return (int)ranks.size() - 1;
  }
  void plan(const double* p, int nq_, long long n) {
    nq = nq_;
    median = nq == 1 && p[0] == 0.5;
    k.resize(nq); kp1.resize(nq); r.resize(nq); ik.resize(nq); ikp1.resize(nq);
    for (int q = 0; q < nq; ++q) {
      if (median) {
        k[q] = (n % 2) ? (n + 1) / 2 : n / 2;                                             // :42, :44
        kp1[q] = (n % 2) ? k[q] : n / 2 + 1;
        r[q] = 0.0;
      } else {
        const double rr = p[q] * (double)n;                                               // :47
        const double kk = std::floor(rr + 0.5);                                           // :48
        r[q] = rr - kk;                                                                   // :50
        k[q] = kk < 1.0 ? 1 : (long long)kk;                                              // :53
        kp1[q] = std::min((long long)kk + 1, n);                                          // :49, :54
      }
      ik[q] = slot(k[q]);
      ikp1[q] = slot(kp1[q]);
    }
  }
  // x: the column's order statistics at `ranks`
  double value(int q, const double* x) const {
    const double xk = x[ik[q]], xk1 = x[ikp1[q]];
    if (median) return k[q] == kp1[q] ? xk : (xk + xk1) / 2.0;                            // :42, :44
    if (r[q] == -0.5 || xk == xk1) return xk;                                             // :60-63, :66-70
    const double u = (0.5 + r[q]) * xk1, v = (0.5 - r[q]) * xk;                           // :57
    return u + v;
  }
};

struct CornerPipeline {
  vbmc_ctx* ctx = nullptr;
  const char* who = "";
  hipStream_t st = nullptr;
  long long Ns = 0;
  int n = 0, nbins = 0, nq = 0, D = 0, P = 0;
  size_t nX = 0;
  bool given = false;
  CornerQuant Q;
  std::vector<int> pairs;
  TmpBuf dX, dB, dCol, dIdx, dHist, dCnt2, dTab, dDens, dTxy, dT, dStat, dPairs, dRank, dSel;

  // everything that can be said of the arguments without the posterior
  vbmc_status begin(vbmc_ctx* ctx_, const char* who_, bool have_vp, const vbmc_corner_args& a) {
    ctx = ctx_; who = who_; st = ctx->stream;
    Ns = a.Ns;
    if (Ns < 2 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 2 .. %lld", who, Ns, VPT_MAXN);
    n = a.res == 0 ? 64 : a.res;
    if (n != 16 && n != 32 && n != 64)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "res = %d: kde2d grids of 16, 32 and 64 are accelerated (one workgroup's LDS tile)", a.res);
    nbins = a.nbins == 0 ? 40 : a.nbins;
    if (nbins < 1 || nbins > CORNER_MAXBINS) return set_err(ctx, VBMC_ERR_INVALID, "%s: nbins = %d outside 1 .. %d", who, a.nbins, CORNER_MAXBINS);
    nq = a.nq;
    if (nq < 0 || nq > CORNER_MAXQ || (nq > 0 && !a.p)) return set_err(ctx, VBMC_ERR_INVALID, "%s: nq = %d outside 0 .. %d, or no p", who, nq, CORNER_MAXQ);
    for (int q = 0; q < nq; ++q)
      if (!(a.p[q] >= 0.0 && a.p[q] <= 1.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: p[%d] is not a probability", who, q);
    if (a.balanceflag != 0 && a.balanceflag != 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: balanceflag %d", who, a.balanceflag);
    given = !have_vp;
    if (have_vp && a.X_in) return set_err(ctx, VBMC_ERR_INVALID, "%s: a posterior and a sample matrix", who);
    if (given) {
      if (!a.X_in) return set_err(ctx, VBMC_ERR_INVALID, "%s: neither a posterior nor a sample matrix", who);
      if (a.D < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: D = %d", who, a.D);
      if (a.D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", a.D, VBMC_LIM_D);
    }
    return VBMC_OK;
  }

  vbmc_status alloc(int D_, const vbmc_corner_args& a) {
    D = D_; P = D * (D - 1) / 2; nX = (size_t)Ns * D;
    if (nX * 8 > ((size_t)1 << 30))
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Ns x D = %lld x %d doubles exceed the 1 GiB the samples may hold on the device", Ns, D);
    if (a.bounds)
      for (int d = 0; d < D; ++d)
        if (!(std::isfinite(a.bounds[2 * d]) && std::isfinite(a.bounds[2 * d + 1]) && a.bounds[2 * d] < a.bounds[2 * d + 1]))
          return set_err(ctx, VBMC_ERR_INVALID, "%s: the bounds of dimension %d are not finite with lo < hi", who, d + 1);
    Q.plan(a.p, nq, Ns);
    pairs.clear();
    for (int d1 = 0; d1 < D - 1; ++d1)                                                    // cornerplot.m:154-155
      for (int d2 = d1 + 1; d2 < D; ++d2) { pairs.push_back(d1); pairs.push_back(d2); }
    const size_t n2 = (size_t)n * n;
    std::vector<double> htab;
    mtv_cos_table(n, htab);
    HIP_TRY(ctx, dX.alloc(ctx, nX * 8));
    HIP_TRY(ctx, dCol.alloc(ctx, (size_t)D * sizeof(CornerCol)));
    HIP_TRY(ctx, dIdx.alloc(ctx, nX));
    HIP_TRY(ctx, dHist.alloc(ctx, (size_t)nbins * D * sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(dHist.p, 0, (size_t)nbins * D * sizeof(int), st));
    if (a.bounds) {
      HIP_TRY(ctx, dB.alloc(ctx, 2 * (size_t)D * 8));
      HIP_TRY(ctx, hipMemcpyAsync(dB.p, a.bounds, 2 * (size_t)D * 8, hipMemcpyHostToDevice, st));
    }
    if (P > 0) {
      HIP_TRY(ctx, dCnt2.alloc(ctx, (size_t)P * n2 * sizeof(int)));
      HIP_TRY(ctx, hipMemsetAsync(dCnt2.p, 0, (size_t)P * n2 * sizeof(int), st));
      HIP_TRY(ctx, dTab.alloc(ctx, htab.size() * 8));
      HIP_TRY(ctx, hipMemcpyAsync(dTab.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, dDens.alloc(ctx, (size_t)P * n2 * 8));
      HIP_TRY(ctx, dTxy.alloc(ctx, 2 * (size_t)P * 8));
      HIP_TRY(ctx, dT.alloc(ctx, (size_t)P * 8));
      HIP_TRY(ctx, dStat.alloc(ctx, (size_t)P * sizeof(int)));
      HIP_TRY(ctx, dPairs.alloc(ctx, pairs.size() * sizeof(int)));
      HIP_TRY(ctx, hipMemcpyAsync(dPairs.p, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    }
    if (!Q.ranks.empty()) {
      HIP_TRY(ctx, dRank.alloc(ctx, Q.ranks.size() * sizeof(int)));
      HIP_TRY(ctx, hipMemcpyAsync(dRank.p, Q.ranks.data(), Q.ranks.size() * sizeof(int), hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, dSel.alloc(ctx, Q.ranks.size() * (size_t)D * 8));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));   // (htab is this function's)
    return VBMC_OK;
  }

  // the samples: the caller's matrix, or vbmc_vp_rnd's rows (vbmc_plot.m:12-15, vbmc_iterplot.m:21, :47)
  vbmc_status upload(const double* X_in) {
    HIP_TRY(ctx, hipMemcpyAsync(dX.p, X_in, nX * 8, hipMemcpyHostToDevice, st));
    return VBMC_OK;
  }
  vbmc_status draw(const VptPack& pk, const VptGenHost& g) {
    VptDrawArgs da{};
    da.P = pk.P; da.G = g.G; da.X = dX.as<double>(); da.I = nullptr;
    VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_draw<DT>), dim3((unsigned)((Ns + VPT_T - 1) / VPT_T)), dim3(VPT_T), 0, st, da))
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  }

  // the launches, the one synchronisation, the host tails, the outputs the caller asked for
  vbmc_status finish(const vbmc_corner_args& a) {
    const size_t n2 = (size_t)n * n;
    const double* x = dX.as<double>();
    {
      CornerRangeArgs r{};
      r.Ns = (int)Ns; r.x = x; r.bounds = a.bounds ? dB.as<double>() : nullptr; r.col = dCol.as<CornerCol>();
      hipLaunchKernelGGL(k_corner_range, dim3(D), dim3(CORNER_T), 0, st, r);
      CornerIndexArgs b{};
      b.Ns = (int)Ns; b.n = n; b.nbins = nbins; b.x = x; b.col = r.col; b.idx = dIdx.as<unsigned char>(); b.hist = dHist.as<int>();
      const unsigned nbx = (unsigned)std::min<long long>((Ns + CORNER_T - 1) / CORNER_T, 64);
      hipLaunchKernelGGL(k_corner_index, dim3(nbx, D), dim3(CORNER_T), 0, st, b);
    }
    if (P > 0) {
      CornerPairsArgs c{};
      c.Ns = (int)Ns; c.n = n; c.idx = dIdx.as<unsigned char>(); c.pairs = dPairs.as<int>(); c.counts2 = dCnt2.as<int>();
      const unsigned nbx = (unsigned)std::max<long long>(1, std::min<long long>(Ns / 8192, 64));
      hipLaunchKernelGGL(k_corner_pairs, dim3(nbx, P), dim3(CORNER_T), 0, st, c);
      CornerKdeArgs k{};
      k.n = n; k.Ns = (int)Ns; k.col = dCol.as<CornerCol>(); k.pairs = c.pairs; k.counts2 = c.counts2; k.tab = dTab.as<double>();
      k.density = dDens.as<double>(); k.txy = dTxy.as<double>(); k.tstar = dT.as<double>(); k.status = dStat.as<int>();
      corner_kde_consts(k);
      hipLaunchKernelGGL(k_corner_kde, dim3(P), dim3(CORNER_T), 0, st, k);
    }
    const int nrank = (int)Q.ranks.size();
    if (nrank > 0) {
      CornerSelectArgs s{};
      s.Ns = (int)Ns; s.nrank = nrank; s.x = x; s.rank = dRank.as<int>(); s.out = dSel.as<double>();
      hipLaunchKernelGGL(k_corner_select, dim3(nrank, D), dim3(CORNER_T), 0, st, s);
    }
    HIP_TRY(ctx, hipGetLastError());

    std::vector<CornerCol> hcol(D);
    std::vector<int> hstat(P), hhist((size_t)nbins * D);
    std::vector<double> htxy(2 * (size_t)P), ht(P), hsel((size_t)nrank * D);
    // the results wait in host vectors until the refusals below are past; the two large ones go straight to the caller
    HIP_TRY(ctx, hipMemcpyAsync(hcol.data(), dCol.p, (size_t)D * sizeof(CornerCol), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hhist.data(), dHist.p, hhist.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (P > 0) {
      HIP_TRY(ctx, hipMemcpyAsync(hstat.data(), dStat.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipMemcpyAsync(htxy.data(), dTxy.p, htxy.size() * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipMemcpyAsync(ht.data(), dT.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
      if (a.density) HIP_TRY(ctx, hipMemcpyAsync(a.density, dDens.p, (size_t)P * n2 * 8, hipMemcpyDeviceToHost, st));
      if (a.counts2) HIP_TRY(ctx, hipMemcpyAsync(a.counts2, dCnt2.p, (size_t)P * n2 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (nrank > 0) HIP_TRY(ctx, hipMemcpyAsync(hsel.data(), dSel.p, hsel.size() * 8, hipMemcpyDeviceToHost, st));
    if (a.xx) HIP_TRY(ctx, hipMemcpyAsync(a.xx, dX.p, nX * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    if (given)
      for (int d = 0; d < D; ++d)
        if (hcol[d].nonfinite) return set_err(ctx, VBMC_ERR_INVALID, "%s: column %d of the sample matrix has an entry that is not finite", who, d + 1);
    for (int pp = 0; pp < P; ++pp)
      if (hstat[pp] == 1)
        return set_err(ctx, VBMC_ERR_UNSUPPORTED,
                       "pair %d, dimensions %d and %d: the bandwidth equation has no bracket below 0.1 (the reference's fminbnd branch, kde2d.m:208-210) -- not accelerated",
                       pp + 1, pairs[2 * pp] + 1, pairs[2 * pp + 1] + 1);
    if (a.bounds_out)
      for (int d = 0; d < D; ++d) { a.bounds_out[2 * d] = hcol[d].MIN; a.bounds_out[2 * d + 1] = hcol[d].MAX; }
    if (a.hist) std::memcpy(a.hist, hhist.data(), hhist.size() * sizeof(int));
    if (a.quant)
      for (int d = 0; d < D; ++d)
        for (int q = 0; q < nq; ++q) a.quant[(size_t)d * nq + q] = Q.value(q, hsel.data() + (size_t)d * nrank);
    for (int pp = 0; pp < P; ++pp) {
      if (a.tstar) a.tstar[pp] = ht[pp];
      if (a.bandwidth) {                                                                  // kde2d.m:107
        const CornerCol &q1 = hcol[pairs[2 * pp]], &q2 = hcol[pairs[2 * pp + 1]];
        a.bandwidth[2 * pp] = std::sqrt(htxy[2 * pp]) * (q1.MAX - q1.MIN);
        a.bandwidth[2 * pp + 1] = std::sqrt(htxy[2 * pp + 1]) * (q2.MAX - q2.MIN);
      }
    }
    return VBMC_OK;
  }
};
}  // namespace

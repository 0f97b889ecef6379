// Host side of the marginal total variation, shared by vbmc_vp_mtv (abi_vp_mtv.hip) and vbmc_vp_diagnostics (abi_vp_diag.hip): the
// constants of fixed_point (kde1d.m:84), the quarter-wave cosine table, the O(n) tail of a column between the inverse transform and
// the integral (kde1d.m:58-62, vbmc_mtv.m:68,71) with its not-a-knot spline system (a serial recurrence), and MtvPipeline: the one
// sequence of checks, allocations, launches, copies back and host sums that takes R runs' draws to their densities and to the
// integrals of pairs of runs.  The entry points keep their argument checks, the packing of the posteriors and the layout of results.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "diag_kernels.h"   // k_diag_dct
#include "mtv_kernels.h"
#include "vp_tools_host.h"  // VptPack, VptGenHost, VPT_FOR_DT

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

// R runs of D columns from their draws to the integrals of pairs of runs.  begin, alloc, add_run once per run in order, finish,
// integrals.  `unit` is what a run is called in a refusal; Args is vbmc_mtv_args or vbmc_diag_args (nkde, nquad, Ns and the stage
// outputs mesh, counts, nuniq, tstar, density are the same fields in both).
// The draws are held in one of two ways.  One run at a time (vbmc_vp_diagnostics: R x 1 GiB would not fit): run i's draws stay valid
// until the next add_run, which launches that run's mesh and counts and copies its draws back.  All at once (vbmc_vp_mtv): mesh and
// counts are one launch each over all R D columns in finish and the draws are copied back there -- per-run launches over D = 10
// columns cost vbmc_vp_mtv 0.18 ms of its 5.6 ms (profiles/mtv_diag_core.md).  The columns are independent: the results are the same.
struct MtvPipeline {
  vbmc_ctx* ctx = nullptr;
  const char *who = "", *unit = "";
  hipStream_t st = nullptr;
  long long Ns = 0;
  int n = 0, nquad = 0, R = 0, D = 0, C = 0;
  size_t nX = 0, nC = 0;
  MtvWork W;                                              // dW's layout
  TmpBuf dX, dEnds, dCol, dNu, dCnt, dW, dTab, dT, dStat;
  std::vector<double> ends, htab, yy, mm, msh;
  std::vector<MtvCol> hcol;
  bool hold_all = false;
  std::vector<double*> xx_out;                            // hold_all: where the caller wants run i's draws, or null

  template <class Args>
  vbmc_status begin(vbmc_ctx* ctx_, const char* who_, const char* unit_, const Args& args) {
    ctx = ctx_; who = who_; unit = unit_; st = ctx->stream;
    Ns = args.Ns;
    if (Ns < 2 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 2 .. %lld", who, Ns, VPT_MAXN);
    n = args.nkde == 0 ? 8192 : args.nkde;
    nquad = args.nquad == 0 ? 100000 : args.nquad;
    if (n < 256 || n > 16384 || (n & (n - 1)) != 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: nkde = %d is not a power of two in 256 .. 16384", who, n);
    if (nquad < 2 || nquad > (1 << 20)) return set_err(ctx, VBMC_ERR_INVALID, "%s: nquad = %d outside 2 .. 2^20", who, nquad);
    return VBMC_OK;
  }

  // pk: the R packed posteriors.  bounded: the mesh is cut at the posterior's bounds (vbmc_mtv.m:55-63 on posteriors); otherwise the
  // bounds are infinite (on sample matrices, :35-38, :44-47).  hold_all: above
  vbmc_status alloc(int R_, int D_, const VptPack* pk, bool bounded, bool hold_all_) {
    R = R_; D = D_; C = R * D; hold_all = hold_all_; xx_out.assign(R, nullptr); nX = (size_t)Ns * D; nC = (size_t)C * n;
    if (nX * 8 > ((size_t)1 << 30))
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Ns x D = %lld x %d doubles per %s exceed the 1 GiB the draws may hold on the device", Ns, D, unit);
    const double inf = std::numeric_limits<double>::infinity();
    ends.resize(4 * (size_t)C);
    for (int i = 0; i < R; ++i) {
      const double* tr = pk[i].L.tr.at(pk[i].h.data());
      for (int d = 0; d < D; ++d) {
        double* e = &ends[4 * ((size_t)i * D + d)];
        e[0] = bounded ? pk[i].lb[d] : -inf;
        e[1] = bounded ? pk[i].ub[d] : inf;
        e[2] = tr ? tr[VPT_ROW_LO * pk[i].DT + d] : -inf;
        e[3] = tr ? tr[VPT_ROW_HI * pk[i].DT + d] : inf;
      }
    }
    mtv_cos_table(n, htab);
    HIP_TRY(ctx, dX.alloc(ctx, (hold_all ? R : 1) * nX * 8));
    HIP_TRY(ctx, dEnds.alloc(ctx, ends.size() * 8));
    HIP_TRY(ctx, dCol.alloc(ctx, (size_t)C * sizeof(MtvCol)));
    HIP_TRY(ctx, dNu.alloc(ctx, (size_t)C * sizeof(long long)));
    HIP_TRY(ctx, dCnt.alloc(ctx, nC * sizeof(int)));
    W = MtvWork(nC);
    HIP_TRY(ctx, dW.alloc(ctx, W.w.bytes()));
    HIP_TRY(ctx, dTab.alloc(ctx, htab.size() * 8));
    HIP_TRY(ctx, dT.alloc(ctx, (size_t)C * 8));
    HIP_TRY(ctx, dStat.alloc(ctx, (size_t)C * sizeof(int)));
    HIP_TRY(ctx, hipMemcpyAsync(dEnds.p, ends.data(), ends.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dTab.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(dCnt.p, 0, nC * sizeof(int), st));
    return VBMC_OK;
  }

  double* run_draws(int i) { return dX.as<double>() + (hold_all ? nX * i : 0); }

  // mesh and counts of the ncol columns from c0 on, whose draws start at x
  void mesh_and_bin(size_t c0, int ncol, const double* x) {
    MtvMeshArgs a{};
    a.Ns = (int)Ns; a.x = x; a.ends = dEnds.as<double>() + 4 * c0; a.col = dCol.as<MtvCol>() + c0; a.nuniq = dNu.as<long long>() + c0;
    hipLaunchKernelGGL(k_mtv_mesh, dim3(ncol), dim3(MTV_T), 0, st, a);
    MtvBinArgs b{};
    b.Ns = (int)Ns; b.n = n; b.x = x; b.col = a.col; b.counts = dCnt.as<int>() + c0 * n;
    const unsigned nbx = (unsigned)std::min<long long>((Ns + MTV_T - 1) / MTV_T, 64);
    hipLaunchKernelGGL(k_mtv_bin, dim3(nbx, ncol), dim3(MTV_T), 0, st, b);
  }

  // run i's draws, vbmc_rnd(vp, Ns, 1, 1) (vbmc_mtv.m:32, :41), exactly vbmc_vp_rnd's rows, wanted at xx if not null
  vbmc_status add_run(int i, const VptPack& pk, const VptGenHost& g, double* xx) {
    VptDrawArgs da{};
    da.P = pk.P; da.G = g.G; da.X = run_draws(i); da.I = nullptr;
    VPT_FOR_DT(pk.DT, hipLaunchKernelGGL((k_vp_draw<DT>), dim3((unsigned)((Ns + VPT_T - 1) / VPT_T)), dim3(VPT_T), 0, st, da))
    xx_out[i] = xx;
    if (!hold_all) {
      mesh_and_bin((size_t)i * D, D, da.X);
      if (xx) HIP_TRY(ctx, hipMemcpyAsync(xx, da.X, nX * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  }

  // over the R D columns: initial data, cosine coefficients, bandwidth, inverse transform (by k_diag_dct if mfma_dct, else by
  // k_mtv_dct); the one synchronisation; the columns' host tail; the stage outputs the caller asked for
  template <class Args>
  vbmc_status finish(bool mfma_dct, const Args& args) {
    double *d_x = W.x.at(dW.p), *d_a = W.a.at(dW.p), *d_a2 = W.a2.at(dW.p), *d_at = W.at.at(dW.p), *d_raw = W.raw.at(dW.p);
    if (hold_all) mesh_and_bin(0, C, dX.as<double>());
    {
      MtvInitArgs c{};
      c.n = n; c.col = dCol.as<MtvCol>(); c.counts = dCnt.as<int>(); c.x = d_x;
      hipLaunchKernelGGL(k_mtv_init, dim3(C), dim3(MTV_T), 0, st, c);
    }
    const size_t lds = ((size_t)n + 1) * 8;
    if (lds > 64 * 1024)
      HIP_TRY(ctx, hipFuncSetAttribute(mfma_dct ? (const void*)k_diag_dct : (const void*)k_mtv_dct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto dct = [&](int inverse, const double* in, double* out, double* a2) {
      MtvDctArgs t{};
      t.n = n; t.inverse = inverse; t.tab = dTab.as<double>(); t.in = in; t.out = out; t.a2 = a2;
      if (mfma_dct) hipLaunchKernelGGL(k_diag_dct, dim3(n / (16 * (DIAG_DCT_T / 64)), (C + 16 * DIAG_DCT_TC - 1) / (16 * DIAG_DCT_TC)), dim3(DIAG_DCT_T), lds, st, t, C);
      else hipLaunchKernelGGL(k_mtv_dct, dim3(n / MTV_T, C), dim3(MTV_T), lds, st, t);
    };
    dct(0, d_x, d_a, d_a2);
    {
      MtvRootArgs a{};
      a.n = n; a.D = D; a.col = dCol.as<MtvCol>(); a.a = d_a; a.a2 = d_a2; a.at = d_at; a.tstar = dT.as<double>(); a.status = dStat.as<int>();
      mtv_root_consts(a);
      hipLaunchKernelGGL(k_mtv_root, dim3(C), dim3(MTV_T), 0, st, a);
    }
    dct(1, d_at, d_raw, nullptr);
    HIP_TRY(ctx, hipGetLastError());

    yy.resize(nC); mm.resize(nC); hcol.resize(C); msh.resize(4 * (size_t)C);
    std::vector<double> ht(C), cp;
    std::vector<int> hstat(C);
    std::vector<long long> hnu(C);
    HIP_TRY(ctx, hipMemcpyAsync(yy.data(), d_raw, nC * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hcol.data(), dCol.p, (size_t)C * sizeof(MtvCol), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hstat.data(), dStat.p, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hnu.data(), dNu.p, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(ht.data(), dT.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
    if (args.counts) HIP_TRY(ctx, hipMemcpyAsync(args.counts, dCnt.p, nC * sizeof(int), hipMemcpyDeviceToHost, st));
    for (int i = 0; hold_all && i < R; ++i)
      if (xx_out[i]) HIP_TRY(ctx, hipMemcpyAsync(xx_out[i], run_draws(i), nX * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int c = 0; c < C; ++c)
      if (hstat[c] == 1)
        return set_err(ctx, VBMC_ERR_UNSUPPORTED,
                       "%s %d, dimension %d: the bandwidth equation has no bracket below 0.1 (the reference's fminbnd branch, kde1d.m:136-138) -- not accelerated",
                       unit, c / D + 1, c % D + 1);
    // kde1d.m:58, :62 and vbmc_mtv.m:68, :71 on the host, then the splines
    for (int c = 0; c < C; ++c) mtv_finish_column(hcol[c], n, yy.data() + (size_t)c * n, mm.data() + (size_t)c * n, &msh[4 * (size_t)c], cp);
    if (args.mesh)
      for (int c = 0; c < C; ++c) { args.mesh[2 * c] = hcol[c].MIN; args.mesh[2 * c + 1] = hcol[c].MAX; }
    if (args.nuniq)
      for (int c = 0; c < C; ++c) args.nuniq[c] = hnu[c];
    if (args.tstar)
      for (int c = 0; c < C; ++c) args.tstar[c] = ht[c];
    if (args.density) std::memcpy(args.density, yy.data(), nC * 8);
    return VBMC_OK;
  }

  // the integrals (vbmc_mtv.m:73-78) of the given pairs of runs (pairs[2 p], pairs[2 p + 1]) in every dimension:
  // out[p D + d], NaN where one of the two columns is bad
  vbmc_status integrals(const std::vector<int>& pairs, std::vector<double>& out) {
    const int npair = (int)(pairs.size() / 2);
    std::vector<double> geo(4 * (size_t)npair * D);
    for (int p = 0; p < npair; ++p)
      for (int d = 0; d < D; ++d) {                                                       // vbmc_mtv.m:74
        double* bb = &geo[4 * ((size_t)p * D + d)];
        const size_t c1 = (size_t)pairs[2 * p] * D + d, c2 = (size_t)pairs[2 * p + 1] * D + d;
        bb[0] = msh[4 * c1]; bb[1] = msh[4 * c1 + 2]; bb[2] = msh[4 * c2]; bb[3] = msh[4 * c2 + 2];
        std::sort(bb, bb + 4);
      }
    const int ntile = (nquad + MTV_T - 1) / MTV_T, nb = std::min(ntile, MTV_NBLK);
    const size_t nent = 3 * (size_t)D * npair;
    const MtvIntBlocks L(nC, msh.size(), geo.size());
    const VptReduceBlock rl((size_t)nb * nent, nent);
    TmpBuf dS, dG, dPr, dP;
    HIP_TRY(ctx, dS.alloc(ctx, L.s.bytes()));
    HIP_TRY(ctx, dG.alloc(ctx, L.g.bytes()));
    HIP_TRY(ctx, dPr.alloc(ctx, pairs.size() * sizeof(int)));
    HIP_TRY(ctx, dP.alloc(ctx, rl.L.bytes()));
    HIP_TRY(ctx, hipMemcpyAsync(L.yy.at(dS.p), yy.data(), L.yy.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.mm.at(dS.p), mm.data(), L.mm.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.msh.at(dG.p), msh.data(), L.msh.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.geo.at(dG.p), geo.data(), L.geo.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dPr.p, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    MtvIntArgs ia{};
    ia.n = n; ia.D = D; ia.nquad = nquad; ia.ntile = ntile; ia.npair = npair; ia.pairs = dPr.as<int>();
    L.bind(ia, dS.p, dG.p);
    ia.partial = rl.partial.at(dP.p);
    double* d_out = rl.out.at(dP.p);
    hipLaunchKernelGGL(k_mtv_integral, dim3(nb, D, npair), dim3(MTV_T), 0, st, ia);
    hipLaunchKernelGGL(k_vp_reduce, dim3((unsigned)((nent + VPT_T - 1) / VPT_T)), dim3(VPT_T), 0, st, ia.partial, nb, (int)nent, d_out);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> ho(nent);
    HIP_TRY(ctx, hipMemcpyAsync(ho.data(), d_out, nent * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    out.assign((size_t)npair * D, std::numeric_limits<double>::quiet_NaN());
    for (int p = 0; p < npair; ++p)
      for (int d = 0; d < D; ++d) {
        const size_t e = (size_t)p * D + d;
        if (hcol[(size_t)pairs[2 * p] * D + d].bad || hcol[(size_t)pairs[2 * p + 1] * D + d].bad) continue;
        double v = 0.0;
        for (int s = 0; s < 3; ++s) {
          const double b0 = geo[4 * e + s], b1 = geo[4 * e + s + 1];
          if (!(b1 > b0)) continue;
          const double x1 = nquad == 2 ? b1 : b0 + (b1 - b0) / (double)(nquad - 1);       // xx_range(2)
          v = v + 0.5 * ho[3 * e + s] * (x1 - b0);                                        // vbmc_mtv.m:77
        }
        out[e] = v;
      }
    return VBMC_OK;
  }
};
}  // namespace

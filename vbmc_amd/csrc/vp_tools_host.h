// Host side of the variational-posterior tools, shared by the entry points that pack a posterior or split a draw (abi_vp_tools.hip,
// abi_vp_mtv.hip, abi_vp_diag.hip, abi_gp_surrogate.hip): validation, the O(D + K) constants of a call (the clamp ends a + eps(a),
// b - eps(b), every log(b - a), log(delta), log(scale), the gammaln constants of the t families, the cumulative weights and counts of
// the draw), one upload per posterior, the dispatch on the padded width.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.h"
#include "vp_tools_kernels.h"

namespace {
constexpr long long VPT_MAXN = 1ll << 28;

inline int vpt_pick_dt(int D) {
  const int dts[] = {4, 8, 12, 16, 24, 32};
  for (int dt : dts)
    if (D <= dt) return dt;
  return 0;
}
inline double vpt_eps(double x) {   // eps(x): the spacing of the doubles at |x|
  x = std::fabs(x);
  return std::nextafter(x, std::numeric_limits<double>::infinity()) - x;
}

#define VPT_FOR_DT(dt_, ...)                                   \
  switch (dt_) {                                               \
    case 4: { constexpr int DT = 4; __VA_ARGS__; } break;      \
    case 8: { constexpr int DT = 8; __VA_ARGS__; } break;      \
    case 12: { constexpr int DT = 12; __VA_ARGS__; } break;    \
    case 16: { constexpr int DT = 16; __VA_ARGS__; } break;    \
    case 24: { constexpr int DT = 24; __VA_ARGS__; } break;    \
    default: { constexpr int DT = 32; __VA_ARGS__; } break;    \
  }

struct VptPack {
  int DT = 0;
  std::vector<double> h, lb, ub;   // the packed block; the bounds (+-Inf without a trinfo) for vbmc_vp_kldiv's comparison
  VptPackLayout L;                 // h's layout, and dev's
  VptPost P{};
  TmpBuf dev;
};

vbmc_status vpt_pack(vbmc_ctx* ctx, const char* who, const vbmc_vp_desc* vp, double df, VptPack& pk) {
  if (!vp || vp->struct_size != sizeof(vbmc_vp_desc)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  const int D = vp->D, K = vp->K;
  if (D < 1 || K < 1) return set_err(ctx, VBMC_ERR_INVALID, "%s: D = %d, K = %d", who, D, K);
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (K > VBMC_LIM_K) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "K = %d > %d not accelerated", K, VBMC_LIM_K);
  if (!vp->mu || !vp->sigma || !vp->lambda || !vp->w) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  bool ok = true;
  double wsum = 0.0, sll = 0.0;
  for (int k = 0; k < K; ++k) {
    ok = ok && std::isfinite(vp->sigma[k]) && vp->sigma[k] > 0.0 && std::isfinite(vp->w[k]) && vp->w[k] >= 0.0;
    wsum += vp->w[k];
    for (int d = 0; d < D; ++d) ok = ok && std::isfinite(vp->mu[d + (size_t)D * k]);
  }
  for (int d = 0; d < D; ++d) { ok = ok && std::isfinite(vp->lambda[d]) && vp->lambda[d] > 0.0; sll += std::log(vp->lambda[d]); }
  if (!ok || !(wsum > 0.0) || !std::isfinite(wsum))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: the variational posterior must be finite with sigma, lambda > 0 and weights >= 0 of positive sum", who);
  const double inf = std::numeric_limits<double>::infinity();
  pk.lb.assign(D, -inf);
  pk.ub.assign(D, inf);
  const bool has_tr = vp->type != nullptr;
  bool has_sc = false;
  double ljc = 0.0;
  if (has_tr) {
    if (!vp->lb || !vp->ub || !vp->tmu || !vp->tdelta) return set_err(ctx, VBMC_ERR_INVALID, "%s: a trinfo needs lb, ub, mu and delta", who);
    for (int d = 0; d < D; ++d) {
      const int t = vp->type[d];
      if (t >= 4 && t <= 13) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "transform type %d of variable %d not accelerated (types 0 .. 3 are)", t, d + 1);
      if (t < 0 || t > 13) return set_err(ctx, VBMC_ERR_INVALID, "%s: transform type %d of variable %d", who, t, d + 1);
      const double a = vp->lb[d], b = vp->ub[d], m = vp->tmu[d], dl = vp->tdelta[d];
      bool good = true;
      if (t == 0 || t == 3) good = good && std::isfinite(m) && std::isfinite(dl) && dl > 0.0;
      if (t == 1 || t == 3) good = good && std::isfinite(a);
      if (t == 2 || t == 3) good = good && std::isfinite(b);
      if (t == 3) good = good && a < b;
      if (!good) return set_err(ctx, VBMC_ERR_INVALID, "%s: bounds, mu or delta of variable %d do not fit its transform type %d", who, d + 1, t);
      pk.lb[d] = a;
      pk.ub[d] = b;
      if (t == 0) ljc += std::log(dl);                                     // warpvars_vbmc.m:487
      if (t == 3) ljc += std::log(b - a) + std::log(dl);                   // :501-502
    }
    if (vp->scale) {
      for (int d = 0; d < D; ++d) {
        if (!(std::isfinite(vp->scale[d]) && vp->scale[d] > 0.0)) return set_err(ctx, VBMC_ERR_INVALID, "%s: scale must be positive", who);
        has_sc = has_sc || vp->scale[d] != 1.0;                            // :67
      }
      if (has_sc) for (int d = 0; d < D; ++d) ljc += std::log(vp->scale[d]);   // :763-765
    }
    if (vp->R)
      for (int e = 0; e < D * D; ++e)
        if (!std::isfinite(vp->R[e])) return set_err(ctx, VBMC_ERR_INVALID, "%s: the rotation must be finite", who);
  }
  const int DT = vpt_pick_dt(D);
  pk.DT = DT;
  VptPost& P = pk.P;
  P.D = D; P.K = K; P.has_tr = has_tr ? 1 : 0; P.has_rot = (has_tr && vp->R) ? 1 : 0; P.has_sc = has_sc ? 1 : 0; P.ljc = ljc;
  const double pi = 3.14159265358979323846;
  if (!std::isfinite(df) || df == 0.0) {
    P.fam = 0; P.dfa = 1.0; P.ce = 0.0;
    P.lognf = -0.5 * D * std::log(2.0 * pi) - sll;                         // vbmc_pdf.m:56
  } else if (df > 0.0) {
    P.fam = 1; P.dfa = df; P.ce = 0.5 * (df + D);
    P.lognf = std::lgamma(0.5 * (df + D)) - std::lgamma(0.5 * df) - 0.5 * D * std::log(df * pi) - sll;               // :75
  } else {
    const double a = -df;
    P.fam = 2; P.dfa = a; P.ce = 0.5 * (a + 1.0);
    P.lognf = D * (std::lgamma(0.5 * (a + 1.0)) - std::lgamma(0.5 * a) - 0.5 * std::log(a * pi)) - sll;              // :93
  }
  pk.L = VptPackLayout(D, DT, K, has_tr);
  const VptPackLayout& L = pk.L;
  pk.h.assign(L.L.count(), 0.0);
  double* h = pk.h.data();
  double *h_mus = L.mus.at(h), *h_cst = L.cst.at(h), *h_is2 = L.is2.at(h), *h_mu = L.mu.at(h), *h_sig = L.sig.at(h);
  for (int k = 0; k < K; ++k) {
    for (int d = 0; d < D; ++d) {
      h_mus[(size_t)k * DT + d] = vp->mu[d + (size_t)D * k] / vp->lambda[d];
      h_mu[d + (size_t)D * k] = vp->mu[d + (size_t)D * k];
    }
    h_cst[k] = vp->w[k] > 0.0 ? std::log(vp->w[k]) - D * std::log(vp->sigma[k]) : -1e300;
    h_is2[k] = 1.0 / (vp->sigma[k] * vp->sigma[k]);
    h_sig[k] = vp->sigma[k];
  }
  for (int d = 0; d < D; ++d) { L.lam.at(h)[d] = vp->lambda[d]; L.ilam.at(h)[d] = 1.0 / vp->lambda[d]; }
  if (has_tr) {
    double* tr = L.tr.at(h);
    for (int d = 0; d < DT; ++d) {
      const bool in = d < D;
      const int t = in ? vp->type[d] : 0;
      const double a = in ? vp->lb[d] : -inf, b = in ? vp->ub[d] : inf;
      tr[VPT_ROW_TYPE * DT + d] = t;
      tr[VPT_ROW_A * DT + d] = a;
      tr[VPT_ROW_B * DT + d] = b;
      tr[VPT_ROW_MU * DT + d] = in && (t == 0 || t == 3) ? vp->tmu[d] : 0.0;
      tr[VPT_ROW_DELTA * DT + d] = in && (t == 0 || t == 3) ? vp->tdelta[d] : 1.0;
      tr[VPT_ROW_SCALE * DT + d] = in && has_sc ? vp->scale[d] : 1.0;
      tr[VPT_ROW_LO * DT + d] = std::isfinite(a) ? a + vpt_eps(a) : a;       // :457
      tr[VPT_ROW_HI * DT + d] = std::isfinite(b) ? b - vpt_eps(b) : b;       // :458
    }
    if (P.has_rot)
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) tr[(size_t)VPT_NROWS * DT + (size_t)i * DT + j] = vp->R[i + (size_t)D * j];
  }
  return VBMC_OK;
}

vbmc_status vpt_upload(vbmc_ctx* ctx, VptPack& pk) {
  HIP_TRY(ctx, pk.dev.alloc(ctx, pk.L.L.bytes()));
  HIP_TRY(ctx, hipMemcpyAsync(pk.dev.p, pk.h.data(), pk.L.L.bytes(), hipMemcpyHostToDevice, ctx->stream));
  pk.L.bind(pk.P, pk.dev.p);
  return VBMC_OK;
}

// the component split and the permutation of a draw (vbmc_rnd.m:57-80); cumulative sums serial, in index order
struct VptGenHost {
  VptGen G{};
  std::vector<double> cdf;
  std::vector<int> cum;
  TmpBuf dcdf, dcum, dB;
};

vbmc_status vpt_gen_host(vbmc_ctx* ctx, const char* who, int K, const double* w, long long N, int balanced, unsigned long long seed, VptGenHost& g) {
  g.cdf.assign(K, 0.0);
  g.cum.assign(K + 1, 0);
  std::vector<double> nf(K);
  long long c = 0;
  for (int k = 0; k < K; ++k) { nf[k] = std::floor(w[k] * (double)N); c += (long long)nf[k]; g.cum[k + 1] = (int)std::min<long long>(c, VPT_MAXN * 2); }
  if (c > 2 * VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: the weights must sum to one", who);
  long long M = N, M0 = 0;
  const double* cw = w;
  std::vector<double> we;
  if (balanced) {
    M0 = c;
    M = M0;
    if (N > M0) {                                      // :67-74
      we.resize(K);
      double se = 0.0;
      for (int k = 0; k < K; ++k) { we[k] = w[k] * (double)N - nf[k]; se = se + we[k]; }
      const double nex = std::ceil(se), de = nex - se;
      for (int k = 0; k < K; ++k) we[k] = we[k] + w[k] * de;
      cw = we.data();
      M = M0 + (long long)nex;
    }
    if (M < N || M > N + K)   // (the dump's caller sizes its block for N + K samples)
      return set_err(ctx, VBMC_ERR_INVALID, "%s: the weights must sum to one (the balanced split has %lld samples for N = %lld)", who, M, N);
  }
  double cs = 0.0;
  for (int k = 0; k < K; ++k) { cs = cs + cw[k]; g.cdf[k] = cs; }
  int hb = 1;
  while ((1ull << (2 * hb)) < (unsigned long long)M) ++hb;
  VptGen& G = g.G;
  G.N = (int)N; G.M = (int)M; G.M0 = (int)M0; G.K = K; G.hb = hb; G.balanced = balanced ? 1 : 0; G.parity = 0; G.origflag = 0; G.seed = seed;
  vpt_keys(seed, G.key);
  return VBMC_OK;
}

vbmc_status vpt_gen_upload(vbmc_ctx* ctx, const char* who, int D, const double* block, VptGenHost& g) {
  const int K = g.G.K;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, g.dcdf.alloc(ctx, (size_t)K * 8));
  HIP_TRY(ctx, g.dcum.alloc(ctx, (size_t)(K + 1) * sizeof(int)));
  HIP_TRY(ctx, hipMemcpyAsync(g.dcdf.p, g.cdf.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(g.dcum.p, g.cum.data(), (size_t)(K + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  g.G.cdf = g.dcdf.as<double>();
  g.G.cum = g.dcum.as<int>();
  if (block) {
    const size_t nB = (size_t)(D + 1) * (size_t)g.G.M;
    for (size_t j = 0; j < nB; ++j) {
      const double v = block[j];
      if (j % (size_t)(D + 1) == 0 ? !(v > 0.0 && v < 1.0) : !std::isfinite(v))
        return set_err(ctx, VBMC_ERR_INVALID, "%s: block value %zu: the uniforms must lie strictly inside (0, 1), the normals must be finite", who, j);
    }
    HIP_TRY(ctx, g.dB.alloc(ctx, nB * 8));
    HIP_TRY(ctx, hipMemcpyAsync(g.dB.p, block, nB * 8, hipMemcpyHostToDevice, st));
    g.G.B = g.dB.as<double>();
    g.G.parity = 1;
  }
  return VBMC_OK;
}

// warpvars_vbmc.m:284-320, :456-459 for one point on the host (the centre of the moments' shifted sums)
void vpt_host_inverse(const vbmc_vp_desc* vp, const VptPack& pk, const double* y, double* x) {
  const int D = vp->D;
  if (!pk.P.has_tr) { for (int d = 0; d < D; ++d) x[d] = y[d]; return; }
  std::vector<double> v(y, y + D), u(D);
  if (pk.P.has_sc) for (int d = 0; d < D; ++d) v[d] *= vp->scale[d];
  for (int i = 0; i < D; ++i) {
    if (!pk.P.has_rot) { u[i] = v[i]; continue; }
    double s = 0.0;
    for (int j = 0; j < D; ++j) s += v[j] * vp->R[i + (size_t)D * j];
    u[i] = s;
  }
  const double* tr = pk.L.tr.at(pk.h.data());
  for (int d = 0; d < D; ++d) {
    const int t = vp->type[d];
    const double a = vp->lb[d], b = vp->ub[d];
    double z;
    if (t == 0) z = u[d] * vp->tdelta[d] + vp->tmu[d];
    else if (t == 1) z = std::exp(u[d]) + a;
    else if (t == 2) z = b - std::exp(u[d]);
    else z = a + (b - a) / (1.0 + std::exp(-(u[d] * vp->tdelta[d] + vp->tmu[d])));
    x[d] = std::min(std::max(z, tr[VPT_ROW_LO * pk.DT + d]), tr[VPT_ROW_HI * pk.DT + d]);
  }
}

inline bool vpt_heavy(double df) { return std::isfinite(df) && df != 0.0; }
}  // namespace

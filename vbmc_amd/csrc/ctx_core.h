// What the entry points share around a context and a surrogate handle: the creation of a context (a caller's, or a child behind the
// pipeline slots), a surrogate assembled from host or device blocks with its per-sample constants, and the surrogate behind an
// entropy-only call.  The entry points themselves are abi_ctx.hip's; users: abi_gp.hip, abi_elbo.hip, elbo_slots.h.
#pragma once
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "elbo_kernels.h"         // GPC_STRIDE
#include "gp_factor_kernels.h"    // k_negate_copy
#include "trsm_mfma.h"            // k_diag_inv, TRSM_NBLK

// with_aux: the second stream is created WITH the context (a caller's context: its blocking calls fork the expected log joint onto it);
// a child behind the pipeline slots never forks and holds one stream.  Created beside the first stream, not on first use: a
// low-priority stream that comes into being after the slot streams no longer yields to the first stream's kernel (the blocking call
// at the headline shape 2.50 -> 2.64 ms, tools/archive/r4_blocking_probe.py).
static vbmc_status ctx_create_impl(int device, void* stream, vbmc_ctx** out, bool with_aux) {
  if (!out) return VBMC_ERR_INVALID;
  *out = nullptr;
  // The pipelined step keeps up to five streams of a context busy (the two pass streams behind the four slots, the exchange stream of a
  // communicator, the context's own and its forked log joint); the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware
  // queues (four by default), and two busy streams that share a queue run one after the other (profiles/r04_experiments.md section 11:
  // the R = 8 step 0.34 -> 0.51 ms when that happens).  The runtime reads the variable when it initialises -- at the first HIP call of the
  // process -- so it is raised HERE, ahead of this function's own first HIP call, for every host alike (the MEX gateway, ctypes, a C
  // caller).  A value already in the environment is kept; it has no effect when another HIP user (torch, say) initialised the runtime
  // first -- the streams are then placed among the queues that exist (stream_beside) -- and VBMC_HW_QUEUES=0 leaves the variable alone.
  // ONCE per process (it ran on every context creation -- setenv from a library races with getenv in the host's other
  // threads, the MATLAB JVM's among them -- so the window is the first creation only, before this library has made any HIP call).
  {
    static std::once_flag hq_once;
    std::call_once(hq_once, [] {
      const char* hq = getenv("VBMC_HW_QUEUES");
      if (!(hq && !strcmp(hq, "0"))) (void)setenv("GPU_MAX_HW_QUEUES", hq && atoi(hq) > 0 ? hq : "8", 0);
    });
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VBMC_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return VBMC_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return VBMC_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return VBMC_ERR_NO_DEVICE;  // gfx950 only, no fallback
  vbmc_ctx* ctx = new vbmc_ctx();
  ctx->device = device;
  ctx->num_cu = prop.multiProcessorCount;
  if (hipSetDevice(device) != hipSuccess) { delete ctx; return VBMC_ERR_HIP; }
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return VBMC_ERR_HIP; }
    ctx->own_stream = true;
  }
  for (auto& e : ctx->ev)
    if (hipEventCreate(&e) != hipSuccess) { delete ctx; return VBMC_ERR_HIP; }
  ctx->overlap = with_aux;
  if (with_aux) (void)ctx_aux(ctx);
  if (hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
    delete ctx;
    return VBMC_ERR_HIP;
  }
  *out = ctx;
  return VBMC_OK;
}

// derived per-sample constants of a surrogate (gplogjoint.m:99-121): S x GPC_STRIDE(D)
static void gp_constants(int D, int S, int Nhyp, int Ncov, int Nnoise, int meanfun, const double* hyp, double* gpc) {
  for (int s = 0; s < S; ++s) {
    const double* h = hyp + (size_t)s * Nhyp;
    double* g = gpc + (size_t)s * GPC_STRIDE(D);
    double sum_lnell = 0.0;
    for (int d = 0; d < D; ++d) {
      double ell = std::exp(h[d]);
      g[d] = ell * ell;
      sum_lnell += h[d];
    }
    const int mo = Ncov + Nnoise;
    for (int d = 0; d < D; ++d) {
      if (meanfun == 4) {
        g[D + d] = h[mo + 1 + d];
        double om = std::exp(h[mo + D + 1 + d]);
        g[2 * D + d] = 1.0 / (om * om);
      } else {
        g[D + d] = 0.0;
        g[2 * D + d] = 0.0;
      }
    }
    g[3 * D] = 2.0 * h[D] + sum_lnell;
    g[3 * D + 1] = meanfun > 0 ? h[mo] : 0.0;
  }
}

// L comes either from the host (L) or, for a posterior just computed on the device (vbmc_gp_post), from device memory:
// dL_chol holds the Cholesky factors (all samples), dL_inv the solves L\(L'\I) of the low-noise samples (negated here).
static vbmc_status gp_upload_impl(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int Ncov, int Nnoise,
                                  int meanfun, const double* X, const double* hyp, const double* alpha,
                                  const double* L, const double* dL_chol, const double* dL_inv, const double* sW1,
                                  const uint8_t* Lchol, vbmc_gp** out) {
  if (!ctx || !out) return VBMC_ERR_INVALID;
  *out = nullptr;
  if (N <= 0 || D <= 0 || S <= 0 || !X || !hyp || !alpha || !sW1)
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_upload: N, D, S must be positive and X/hyp/alpha/sW1 non-null");
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "vbmc_gp_upload: D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (!(meanfun == 0 || meanfun == 1 || meanfun == 4))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "gplogjoint:UnsupportedMeanFun: meanfun %d not accelerated (0,1,4 are)", meanfun);
  if (Ncov != D + 1) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "only the SE-ARD covariance (Ncov = D+1) is accelerated");
  const int Nmean = meanfun == 0 ? 0 : (meanfun == 1 ? 1 : 2 * D + 1);
  if (Nhyp < Ncov + Nnoise + Nmean)
    return set_err(ctx, VBMC_ERR_INVALID, "gplite_post:dimmismatch: Nhyp = %d < Ncov+Nnoise+Nmean = %d", Nhyp, Ncov + Nnoise + Nmean);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  vbmc_gp* gp = new vbmc_gp();
  gp->N = N; gp->D = D; gp->S = S; gp->Nhyp = Nhyp; gp->Ncov = Ncov; gp->Nnoise = Nnoise; gp->meanfun = meanfun;
  gp->hyp_host.assign(hyp, hyp + (size_t)Nhyp * S);
  gp->sn2_eff.resize(S);
  gp->Lchol.resize(S);
  for (int s = 0; s < S; ++s) {
    gp->sn2_eff[s] = 1.0 / (sW1[s] * sW1[s]);  // gplogjoint.m:160
    gp->Lchol[s] = Lchol ? Lchol[s] : 1;
  }
  std::vector<double> gpc((size_t)S * GPC_STRIDE(D));
  gp_constants(D, S, Nhyp, Ncov, Nnoise, meanfun, hyp, gpc.data());
  // device blocks of a surrogate come from the context's pool (hipMalloc / hipFree cost ~0.1 ms each and serialise the
  // device: an append or a re-upload per acquired point would pay for a dozen of them)
  gp->pooled = true;
  // uploads are queued on the context's stream and awaited once at the end (every source outlives this function's last
  // synchronisation): a blocking hipMemcpy per array cost ~50 us each, seven of them per surrogate
  auto up = [&](double** dst, const double* src, size_t n) -> hipError_t {
    hipError_t e = pool_get(ctx, n * sizeof(double), (void**)dst);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(*dst, src, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  };
  hipError_t e = up(&gp->X, X, (size_t)N * D);
  if (e == hipSuccess) e = up(&gp->alpha, alpha, (size_t)N * S);
  if (e == hipSuccess) e = up(&gp->gpc, gpc.data(), gpc.size());
  if (e == hipSuccess) e = up(&gp->hyp, hyp, (size_t)Nhyp * S);
  if (e == hipSuccess && L) {
    e = up(&gp->L, L, (size_t)N * N * S);
    gp->hasL = true;
  } else if (e == hipSuccess && dL_chol) {
    e = pool_get(ctx, (size_t)N * N * S * sizeof(double), (void**)&gp->L);
    if (e == hipSuccess && !dL_inv) {       // every sample on the Cholesky branch: one contiguous copy
      e = hipMemcpyAsync(gp->L, dL_chol, (size_t)S * N * N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
    } else {
      for (int s = 0; s < S && e == hipSuccess; ++s) {
        const size_t off = (size_t)s * N * N;
        if (gp->Lchol[s]) e = hipMemcpyAsync(gp->L + off, dL_chol + off, (size_t)N * N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        else hipLaunchKernelGGL(k_negate_copy, dim3((unsigned)(((size_t)N * N + 255) / 256)), dim3(256), 0, ctx->stream, (size_t)N * N, dL_inv + off, gp->L + off);
      }
    }
    gp->hasL = true;
  }
  if (e == hipSuccess) e = up(&gp->d_sn2, gp->sn2_eff.data(), (size_t)S);
  std::vector<double> mx(D);          // function scope: its copy is queued, not awaited, below
  if (e == hipSuccess) {
    for (int d = 0; d < D; ++d) {
      double acc = 0.0;
      for (int n = 0; n < N; ++n) acc += X[n + (size_t)N * d];
      mx[d] = acc / N;
    }
    e = up(&gp->d_meanX, mx.data(), (size_t)D);
  }
  if (e == hipSuccess) {
    e = pool_get(ctx, (size_t)S, (void**)&gp->d_lchol);
    if (e == hipSuccess) e = hipMemcpyAsync(gp->d_lchol, gp->Lchol.data(), (size_t)S, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess && gp->hasL) {
    e = pool_get(ctx, (size_t)S * TRSM_NBLK(N) * 256 * sizeof(double), (void**)&gp->d_finv);
    if (e == hipSuccess) hipLaunchKernelGGL(k_diag_inv, dim3(TRSM_NBLK(N), S), dim3(64), 0, ctx->stream, N, gp->L, gp->d_lchol, gp->d_finv);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the one wait for everything queued above
  else (void)hipStreamSynchronize(ctx->stream);                   // sources of queued copies die with this frame
  if (e != hipSuccess) {
    vbmc_gp_free(ctx, gp);
    return set_err(ctx, VBMC_ERR_HIP, "vbmc_gp_upload: %s", hipGetErrorString(e));
  }
  *out = gp;
  return VBMC_OK;
}

// The surrogate behind an entropy-only call: N = 1, alpha = 0, meanfun 0  =>  G = 0 and dG = 0 exactly, so that
// H, dH (and F = -H + penalties) are entmc_vbmc / entlb_vbmc on their own (ent/entmc_vbmc.m:1, ent/entlb_vbmc.m:1).
static vbmc_status null_gp_for(vbmc_ctx* ctx, int D, const vbmc_gp** out) {
  if (D <= 0 || D > 32) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", D);
  if (!ctx->null_gp[D]) {
    std::vector<double> X(D, 0.0), hyp(D + 2, 0.0);
    const double alpha = 0.0, sW1 = 1.0;
    const uint8_t lchol = 1;
    VB_TRY(gp_upload_impl(ctx, 1, D, 1, D + 2, D + 1, 1, 0, X.data(), hyp.data(), &alpha, nullptr, nullptr, nullptr, &sW1, &lchol, &ctx->null_gp[D]));
  }
  *out = ctx->null_gp[D];
  return VBMC_OK;
}

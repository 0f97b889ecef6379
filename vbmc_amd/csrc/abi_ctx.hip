// C-ABI entry points of libvbmc_hip.so around the context (include/vbmc_hip.h): its lifetime, synchronisation and profiling, raw device
// memory, the upload of a GP surrogate, vbmc_get_limits and the test hooks.
#include "elbo_pass.h"

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
extern "C" int vbmc_abi_version(void) { return VBMC_ABI_VERSION; }

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
extern "C" vbmc_status vbmc_ctx_create(int device, void* stream, vbmc_ctx** out) { return ctx_create_impl(device, stream, out, true); }

extern "C" void vbmc_ctx_destroy(vbmc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  DevBuf* bufs[] = {&ctx->theta, &ctx->prep, &ctx->entp, &ctx->ljpart, &ctx->entpart, &ctx->out,
                    &ctx->eps, &ctx->bnd, &ctx->vpfix, &ctx->misc, &ctx->varbuf, &ctx->zbuf};
  for (DevBuf* b : bufs)
    if (b->p) (void)hipFree(b->p);
  for (auto& b : ctx->pool)
    if (b.p) (void)hipFree(b.p);
  for (vbmc_gp* g : ctx->null_gp) vbmc_gp_free(ctx, g);
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  for (int sl = 0; sl < 2; ++sl) {
    if (ctx->slot_pin[sl]) (void)hipHostFree(ctx->slot_pin[sl]);
    if (ctx->slot_ev[sl]) (void)hipEventDestroy(ctx->slot_ev[sl]);
    delete (SlotPlan*)ctx->slot_plan[sl];
  }
  for (auto& e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  for (vbmc_ctx* sc : ctx->slot_sub)
    if (sc) vbmc_ctx_destroy(sc);
  for (int sl = 0; sl < VBMC_SLOTS; ++sl) {
    if (ctx->slot_xev[sl]) (void)hipEventDestroy(ctx->slot_xev[sl]);
    if (ctx->slot_yev[sl]) (void)hipEventDestroy(ctx->slot_yev[sl]);
    if (ctx->slot_zev[sl]) (void)hipEventDestroy(ctx->slot_zev[sl]);
  }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" const char* vbmc_last_error(const vbmc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" vbmc_status vbmc_ctx_synchronize(vbmc_ctx* ctx) {
  if (!ctx) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (vbmc_ctx* sc : ctx->slot_sub)
    if (sc) HIP_TRY(ctx, hipStreamSynchronize(sc->stream));
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_ctx_set_profiling(vbmc_ctx* ctx, int enable) {
  if (!ctx) return VBMC_ERR_INVALID;
  ctx->profiling = enable != 0;
  ctx->prof_alone = enable == 2;
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_ctx_last_kernel_ms(vbmc_ctx* ctx, double* ent_ms, double* logjoint_ms) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (ent_ms) *ent_ms = ctx->last_ent_ms;
  if (logjoint_ms) *logjoint_ms = ctx->last_lj_ms;
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_ctx_last_launch(vbmc_ctx* ctx, int* ent_form, int* lj_form) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (ent_form) *ent_form = ctx->last_ent_form;
  if (lj_form) *lj_form = ctx->last_lj_form;
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_device_alloc(vbmc_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMalloc(dptr, bytes));
  return VBMC_OK;
}
extern "C" vbmc_status vbmc_device_free(vbmc_ctx* ctx, void* dptr) {
  if (!ctx) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipFree(dptr));
  return VBMC_OK;
}
extern "C" vbmc_status vbmc_memcpy_h2d(vbmc_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VBMC_OK;
}
extern "C" vbmc_status vbmc_memcpy_d2h(vbmc_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// GP upload
// ------------------------------------------------------------------------------------------
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

extern "C" vbmc_status vbmc_gp_upload(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int Ncov, int Nnoise,
                                      int meanfun, const double* X, const double* hyp, const double* alpha,
                                      const double* L, const double* sW1, const uint8_t* Lchol,
                                      vbmc_gp** out) {
  return gp_upload_impl(ctx, N, D, S, Nhyp, Ncov, Nnoise, meanfun, X, hyp, alpha, L, nullptr, nullptr, sW1, Lchol, out);
}

extern "C" void vbmc_gp_free(vbmc_ctx* ctx, vbmc_gp* gp) {
  if (!gp) return;
  if (ctx && gp->pooled) ctx_drain_slots(ctx);   // a pass in flight on a slot stream may still read the blocks the pool is about to hand out again
  // pooled blocks go back to the context's pool; without a live context (destroyed first) they are already gone with it
  // in_views: X, hyp, gpc, d_sn2, d_lchol, d_mult, d_meanX are windows into blk_in (a posterior assembled by vbmc_gp_post from
  // its own packed upload, gp_factor.h)
  void* blocks[] = {gp->in_views ? nullptr : gp->X, gp->alpha, gp->L, gp->in_views ? nullptr : gp->gpc, gp->in_views ? nullptr : gp->hyp,
                    gp->in_views ? nullptr : gp->d_sn2, gp->in_views ? nullptr : gp->d_lchol, gp->in_views ? nullptr : gp->d_mult,
                    gp->d_finv, gp->d_tinv, gp->in_views ? nullptr : gp->d_meanX, gp->blk_in};
  for (void* b : blocks) {
    if (!b) continue;
    if (gp->pooled) { if (ctx) pool_put(ctx, b); }
    else (void)hipFree(b);
  }
  delete gp;
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

// ------------------------------------------------------------------------------------------
// limits and test hooks
// ------------------------------------------------------------------------------------------
// largest variational parameter count whose five T-vectors fit k_var_final's LDS (with S = 1, K = 1: the bound elbo_plan applies per call)
static int limit_T_vargrad() {
  int T = 1;
  while (VAR_FINAL_LDS(1, 1, T + 1) <= 160 * 1024) ++T;
  return T;
}
extern "C" vbmc_status vbmc_get_limits(vbmc_limits* out) {
  if (!out || out->struct_size != sizeof(vbmc_limits)) return VBMC_ERR_INVALID;
  out->max_D = VBMC_LIM_D;
  out->max_K = VBMC_LIM_K;
  out->max_N = trsm_max_n();
  out->max_Na = VBMC_LIM_NA;
  out->max_T_vargrad = limit_T_vargrad();
  out->delta_ok = 1;
  out->meanfun_mask = VBMC_LIM_MEANFUN_MASK;
  return VBMC_OK;
}

// test / reporting hook: the instantiation the Monte-Carlo entropy of a D-dimensional K-component mixture runs on (dense mode):
// qs = ceil((D + 2) / 4), kt = k-tiles per wave, hv = waves per workgroup, tail = tail values per lane (0: none).  Returns 0 when
// the matrix-core kernel does not serve the shape (the VALU kernel does).
extern "C" int vbmc_entropy_plan(int D, int K, int* qs, int* kt, int* hv, int* tail) {
  if (lane_entropy_fits(D, K, 0.0)) {       // small mixtures: k_entropy_lane<DT, KP> (qs: DT, kt: KP, four waves per workgroup)
    if (qs) *qs = 2 * ((D + 1) / 2);
    if (kt) *kt = 2 * ((K + 1) / 2);
    if (hv) *hv = ENT_LANE_WAVES_HOST;
    if (tail) *tail = 0;
    return 2;
  }
  int q = 0, k = 0, h = 0;
  const bool ok = mfma_entropy_fits(D, K, 0.0, read_launch_switches(), &q, &k, &h);
  if (qs) *qs = q;
  if (kt) *kt = k;
  if (hv) *hv = h & 15;
  if (tail) *tail = h >> 4;
  return ok ? 1 : 0;
}

#ifdef VBMC_INSTRUMENT
extern "C" int vbmc_dbg_fin_read(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_dbg), 64 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

// test hook: y[i] = exp(x[i]) with the hot-loop implementations (variant 0: vb_exp, 1: vb_exp_tab<0>, 2: vb_exp_tab<1>)
__global__ void k_test_exp(int n, int variant, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double tab[VB_EXP_TAB_N];
  for (int t = threadIdx.x; t < VB_EXP_TAB_N; t += blockDim.x) tab[t] = c_exp2_tab[t];
  __syncthreads();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = variant == 2 ? vb_exp_tab<1>(x[i], tab) : (variant ? vb_exp_tab<0>(x[i], tab) : vb_exp(x[i]));
}

// variant 3: vb_exp_tab1k, the entropy kernel's exp, on y = x * 1024/ln2 (in the kernel the factor sits in the MFMA operands)
#include "exp2_tab1k.h"
// variant 3: as the entropy kernel is built (VB_EXP_TAB1K_QUAD), 4: the economised cubic, 5: the economised quadratic
__global__ void k_test_exp1k(int n, int variant, const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double tab[VB_EXP_TAB1K_N];
  for (int t = threadIdx.x; t < VB_EXP_TAB1K_N; t += blockDim.x) tab[t] = c_exp2_tab1k[t];
  __syncthreads();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    double ys;   // a ROUNDED product, as the MFMA delivers it: the compiler must not contract it into the reduction's subtraction
    asm volatile("v_mul_f64 %0, %1, %2" : "=v"(ys) : "v"(x[i]), "v"(VB_EXP_TAB1K_SCALE));
    const bool quad = variant == 3 ? VB_EXP_TAB1K_QUAD : variant == 5;
    y[i] = quad ? vb_exp_tab1k<true>(ys, tab) : vb_exp_tab1k<false>(ys, tab);
  }
}

extern "C" vbmc_status vbmc_test_exp(vbmc_ctx* ctx, int n, int variant, const double* x, double* y) {
  if (!ctx || n <= 0 || !x || !y) return VBMC_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  VB_TRY(ensure(ctx, ctx->misc, 2 * (size_t)n * sizeof(double)));
  double* dx = (double*)ctx->misc.p;
  HIP_TRY(ctx, hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (variant >= 3 && variant <= 5) hipLaunchKernelGGL(k_test_exp1k, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, variant, dx, dx + n);
  else if (variant < 0 || variant > 5) return VBMC_ERR_INVALID;
  else hipLaunchKernelGGL(k_test_exp, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, variant, dx, dx + n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(y, dx + n, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_rng_dump(vbmc_ctx* ctx, int D, int K, int R, int Ns, uint64_t seed, double* eps_host) {
  if (!ctx || !eps_host || D <= 0 || K <= 0 || R <= 0 || Ns <= 0) return VBMC_ERR_INVALID;
  const int Mh = (Ns + 1) / 2;
  const size_t n = (size_t)D * Mh * K * R;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  VB_TRY(ensure(ctx, ctx->eps, n * sizeof(double)));
  const long long total = (long long)R * K * Mh;
  hipLaunchKernelGGL(k_rng_dump, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, D, K, R, Mh,
                     (unsigned long long)seed, (double*)ctx->eps.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(eps_host, ctx->eps.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VBMC_OK;
}

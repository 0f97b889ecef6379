// C-ABI entry points of libvbmc_hip.so around the context (include/vbmc_hip.h): its lifetime, synchronisation and profiling, raw device
// memory, the upload of a GP surrogate, vbmc_get_limits and the test hooks.
#include "ctx_core.h"
#include "elbo_pass.h"

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
extern "C" int vbmc_abi_version(void) { return VBMC_ABI_VERSION; }

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

extern "C" vbmc_status vbmc_ctx_last_variance(vbmc_ctx* ctx, vbmc_var_launch_info* out) {
  if (!ctx || !out) return VBMC_ERR_INVALID;
  if (out->struct_size != sizeof(vbmc_var_launch_info))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_var_launch_info.struct_size %u != %zu (ABI mismatch)", out->struct_size, sizeof(vbmc_var_launch_info));
  *out = ctx->last_var;
  out->struct_size = sizeof(vbmc_var_launch_info);
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

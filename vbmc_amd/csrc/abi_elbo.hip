// C-ABI entry points of libvbmc_hip.so for the ELBO objective (include/vbmc_hip.h): the blocking batch, the sharded evaluation and the
// on-device Adam loop.  The pass itself -- plan, stages, read-back -- is elbo_pass.h; the pipelined form is abi_elbo_slots.hip.
#include "ctx_core.h"    // null_gp_for: the entropy-only call
#include "elbo_pass.h"

// ------------------------------------------------------------------------------------------
// vbmc_elbo_batch
// ------------------------------------------------------------------------------------------
extern "C" vbmc_status vbmc_elbo_batch(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!gp && a) {  // entropy only
    if (a->compute_var != 0 || a->separate_K)
      return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_batch: an entropy-only call (gp == NULL) has no variance / per-component outputs");
    VB_TRY(null_gp_for(ctx, a->D, &gp));
  }
  ElboPlan P;
  VB_TRY(elbo_plan(ctx, gp, a, P));
  const size_t ndvs = a->dvarG_s ? (size_t)P.dm.T * P.dm.S * P.dm.R : 0;    // gplogjoint's dvarF with avg_flag = 0: T x S per restart
  TmpBuf dvs;                                                               // (held until the stream has been waited for, on every path below)
  if (ndvs) HIP_TRY(ctx, dvs.alloc(ctx, ndvs * sizeof(double)));
  P.d_dvs = dvs.as<double>();
  vbmc_status st = elbo_enqueue(ctx, gp, P, a->seed);
  if (!st) st = elbo_read_results(ctx, P, a);      // (waits for the stream)
  if (P.d_dvs && st) (void)hipStreamSynchronize(ctx->stream);
  if (P.d_dvs && !st) {
    hipError_t e_ = hipMemcpy(a->dvarG_s, P.d_dvs, ndvs * sizeof(double), hipMemcpyDeviceToHost);
    if (e_ != hipSuccess) { (void)hipGetLastError(); st = set_err(ctx, VBMC_ERR_HIP, "per-hyper-sample variance gradient read-back: %s", hipGetErrorString(e_)); }
  }
  return st;
}

// ------------------------------------------------------------------------------------------
// one evaluation sharded over `world` ranks along the hyper-sample axis and the entropy sample chunks (elbo_pass.h: ShardSpec)
// ------------------------------------------------------------------------------------------
static vbmc_status shard_plan(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int rank, int world, ElboPlan& P) {
  if (!gp || !a) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_shard_*: null gp / args");
  if (world < 1 || rank < 0 || rank >= world) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_shard_*: rank %d of world %d", rank, world);
  if (a->compute_var != 0 || a->separate_K || a->G_s || a->varG_s || a->dG_s || a->dvarG_s)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "vbmc_elbo_shard_*: the sharded evaluation covers value + gradient without variance "
                                              "(the optimiser-loop call, misc/vpoptimize_vbmc.m:71)");
  if (a->eps_mode != 0 && a->Ns > 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "vbmc_elbo_shard_*: device RNG only (eps_mode 0)");
  return elbo_plan(ctx, gp, a, P, world);
}

extern "C" vbmc_status vbmc_elbo_shard_size(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int world, size_t* n_doubles) {
  if (!ctx || !n_doubles) return VBMC_ERR_INVALID;
  ElboPlan P;
  VB_TRY(shard_plan(ctx, gp, a, 0, world, P));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_doubles = shard_doubles(P, world);
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_elbo_shard_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int rank, int world,
                                             double* d_send) {
  if (!ctx || !d_send) return VBMC_ERR_INVALID;
  ElboPlan P;
  VB_TRY(shard_plan(ctx, gp, a, rank, world, P));
  PassOpts o;
  o.shard.mode = 1; o.shard.rank = rank; o.shard.world = world; o.shard.send = d_send;
  HIP_TRY(ctx, hipMemsetAsync(d_send, 0, shard_doubles(P, world) * sizeof(double), ctx->stream));   // unused slots of an uneven split
  VB_TRY(elbo_enqueue(ctx, gp, P, a->seed, o));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the exchange runs on the caller's stream / communicator
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_elbo_shard_finish(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, int world,
                                              const double* d_gathered) {
  if (!ctx || !d_gathered) return VBMC_ERR_INVALID;
  ElboPlan P;
  VB_TRY(shard_plan(ctx, gp, a, 0, world, P));
  PassOpts o;
  o.shard.mode = 2; o.shard.world = world; o.shard.gathered = d_gathered;
  VB_TRY(elbo_enqueue(ctx, gp, P, a->seed, o));
  return elbo_read_results(ctx, P, a);
}

// ------------------------------------------------------------------------------------------
// On-device Adam (utils/fminadam.m:42-102) for R chains in lock-step: the whole loop
// [ELBO+grad pass -> Adam update -> every 20 iterations the slope / random-walk stopping test]
// is enqueued on the stream without host round trips; the host only polls R "done" flags every
// 20 iterations (the reference tests termination on exactly those iterations, fminadam.m:65).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_adam_step(AdamState A, int iter, double* __restrict__ x /*T x R*/,
                                                   const double* __restrict__ out /*R x (5+3T)*/) {
  adam_update_chain(A, iter, x, out, blockIdx.x);
}

// stopping test at iter (a multiple of 20, >= 40): fminadam.m:65-81
__global__ void __launch_bounds__(256) k_adam_check(AdamState A, int iter) {
  __shared__ double red[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (A.done[r]) return;
  const int T = A.T, B = 20;
  const double* f = A.ftab + (size_t)r * A.MaxIter + (iter - B);
  // dx = sqrt(sum((mean(x last B) - mean(x previous B)).^2 / B))
  double part = 0.0;
  for (int i = tid; i < T; i += blockDim.x) {
    double a = 0.0, b = 0.0;
    for (int t = 0; t < B; ++t) {
      a += A.xtab[((size_t)r * A.MaxIter + (iter - B + t)) * T + i];
      b += A.xtab[((size_t)r * A.MaxIter + (iter - 2 * B + t)) * T + i];
    }
    double d = a / B - b / B;
    part += d * d / B;
  }
  red[tid] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
  if (tid == 0) {
    const double dx = sqrt(red[0]);
    // degree-1 least squares on xxp = linspace(-(B-1)/2, (B-1)/2, B): slope and its variance A(1,1) (:66-69)
    double fm = 0.0;
    for (int t = 0; t < B; ++t) fm += f[t];
    fm /= B;
    double sxx = 0.0, sxy = 0.0;
    for (int t = 0; t < B; ++t) { double xx = -(B - 1) / 2.0 + t; sxx += xx * xx; sxy += xx * (f[t] - fm); }
    const double slope = sxy / sxx;
    double rss = 0.0;
    for (int t = 0; t < B; ++t) { double xx = -(B - 1) / 2.0 + t; double e = f[t] - (fm + slope * xx); rss += e * e; }
    const double svar = rss / (B - 2) / sxx;
    const double TolX = 0.001, TolX_max = 0.1, TolFun_max = A.TolFun * 100.0;
    const double slope_err = sqrt(svar + A.TolFun * A.TolFun), slope_err_max = sqrt(svar + TolFun_max * TolFun_max);
    if ((dx < TolX && fabs(slope) < slope_err_max) || (fabs(slope) < slope_err && dx < TolX_max)) A.done[r] = iter;  // :79
  }
}

extern "C" vbmc_status vbmc_adam_batch(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, double TolFun, int MaxIter,
                                       double step_min, double step_max, double step_decay, double* x_out, double* f_out,
                                       int32_t* iters_out, double* xtab_out, double* ftab_out, double* xmid_out) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!a || !a->compute_grad) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_adam_batch needs compute_grad = 1");
  if (MaxIter < 1) return set_err(ctx, VBMC_ERR_INVALID, "MaxIter must be >= 1");
  if (a->eps_mode != 0 && a->Ns > 0) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_adam_batch draws fresh device RNG every iteration (eps_mode 0)");
  if (a->separate_K || a->I_sk || a->J_sjk || a->G_s || a->varG_s || a->dG_s || a->dvarG_s || a->dvarG)      // (accepted by elbo_plan, never served here)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "vbmc_adam_batch: per-component / per-hyper-sample outputs only through vbmc_elbo_batch");
  ElboPlan P;
  VB_TRY(elbo_plan(ctx, gp, a, P));
  const int T = P.dm.T, R = P.dm.R;
  hipStream_t st = ctx->stream;
  const size_t nT = (size_t)T * R, nx = (size_t)T * MaxIter * R, nf = (size_t)MaxIter * R;
  VB_TRY(ensure(ctx, ctx->misc, (2 * nT + nx + nf) * sizeof(double) + (size_t)R * sizeof(int)));
  AdamState A{};
  A.m = (double*)ctx->misc.p; A.v = A.m + nT; A.xtab = A.v + nT; A.ftab = A.xtab + nx; A.done = (int*)(A.ftab + nf);
  A.T = T; A.R = R; A.MaxIter = MaxIter; A.step_min = step_min; A.step_max = step_max; A.step_decay = step_decay; A.TolFun = TolFun;
  HIP_TRY(ctx, hipMemsetAsync(A.m, 0, 2 * nT * sizeof(double), st));
  HIP_TRY(ctx, hipMemsetAsync(A.done, 0, (size_t)R * sizeof(int), st));
  std::vector<int> done(R, 0);
  int iter = 0;
  // the factors of iteration `it`'s update (utils/fminadam.m:53-57), handed to the kernels with the state
  auto adam_set_iter = [&](AdamState& S_, int it) {
    S_.c1 = 1.0 - std::pow(0.9, (double)it); S_.c2 = 1.0 - std::pow(0.999, (double)it);
    S_.step = step_min + (step_max - step_min) * std::exp(-(double)it / step_decay);
  };
  // Where the NEXT iteration follows without a stopping test in between, this iteration's finalize kernel applies the Adam update
  // and unpacks the new theta itself (k_finalize_ws: fused), and the next pass starts at its log-joint kernel; before a stopping
  // test (every 20 iterations from the 40th, utils/fminadam.m:65) and at the end the update is a launch of its own.
  PassOpts o;             // o.skip_prep: the previous pass has already applied its update and unpacked theta for this one
  for (iter = 1; iter <= MaxIter; ++iter) {
    const bool check = iter % 20 == 0 && iter >= 40;
    const bool last = check || iter == MaxIter;
    const bool fuse = !last;
    adam_set_iter(A, iter);
    o.fuse = fuse ? &A : nullptr; o.fuse_iter = iter;
    VB_TRY(elbo_enqueue(ctx, gp, P, a->seed + (unsigned long long)iter, o));
    o.skip_prep = fuse;
    // the stopping test and the final read-back need this iteration's update now; the next pass unpacks theta itself
    if (!fuse) hipLaunchKernelGGL(k_adam_step, dim3(R), dim3(256), 0, st, A, iter, P.d_theta, P.d_out);
    if (check) {
      hipLaunchKernelGGL(k_adam_check, dim3(R), dim3(256), 0, st, A, iter);
      HIP_TRY(ctx, hipMemcpyAsync(done.data(), A.done, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      bool all = true;
      for (int r = 0; r < R; ++r) all = all && done[r] != 0;
      if (all) break;
    }
  }
  if (iter > MaxIter) iter = MaxIter;
  HIP_TRY(ctx, hipGetLastError());
  // outputs: x = mean of the last 20 iterates, f = mean of the last 20 values (fminadam.m:96-97).  Only the iterations that were
  // run come back: `iter` rows of each chain's table (a strided copy), not the MaxIter the table was sized for -- with
  // MaxIter = 1e4 and chains that stop after a few hundred iterations that is the difference between megabytes and hundreds of them
  const size_t nit = (size_t)iter;
  std::vector<double> xt(nit * T * R), ft(nit * R);
  HIP_TRY(ctx, hipMemcpy2DAsync(xt.data(), nit * T * sizeof(double), A.xtab, (size_t)MaxIter * T * sizeof(double), nit * T * sizeof(double), R,
                                hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpy2DAsync(ft.data(), nit * sizeof(double), A.ftab, (size_t)MaxIter * sizeof(double), nit * sizeof(double), R,
                                hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(done.data(), A.done, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int r = 0; r < R; ++r) {
    const int it = done[r] ? done[r] : iter;
    const int nb = it < 20 ? it : 20;
    const double* xr = xt.data() + (size_t)r * nit * T;
    const double* fr = ft.data() + (size_t)r * nit;
    if (iters_out) iters_out[r] = it;
    for (int i = 0; i < T; ++i) {
      double acc = 0.0;
      for (int t = it - nb; t < it; ++t) acc += xr[(size_t)t * T + i];
      if (x_out) x_out[(size_t)r * T + i] = acc / nb;
    }
    double fa = 0.0;
    for (int t = it - nb; t < it; ++t) fa += fr[t];
    if (f_out) f_out[r] = fa / nb;
    if (xmid_out) {   // the iterate with the smallest recorded objective: [~,idx_mid] = min(fval_lst) (misc/vpoptimize_vbmc.m:133; first minimum, NaN skipped)
      int best = 0;
      bool have = false;
      for (int t = 0; t < it; ++t)
        if (!std::isnan(fr[t]) && (!have || fr[t] < fr[best])) { best = t; have = true; }
      memcpy(xmid_out + (size_t)r * T, xr + (size_t)best * T, (size_t)T * sizeof(double));
    }
    if (xtab_out) memcpy(xtab_out + (size_t)r * MaxIter * T, xr, (size_t)it * T * sizeof(double));
    if (ftab_out) memcpy(ftab_out + (size_t)r * MaxIter, fr, (size_t)it * sizeof(double));
  }
  return VBMC_OK;
}

// One ELBO evaluation pass on the host side: the plan (validation, one staged upload, scratch, every launch decision), the stages
// that enqueue it and their driver, the read-back and its unpacking.  The entry points are in abi_elbo.hip (blocking, sharded,
// on-device Adam), abi_elbo_slots.hip (pipeline slots) and abi_comm.hip (communicator).
#pragma once
#include <algorithm>
#include <cmath>
#include <mutex>

#include "elbo_kernels.h"
#include "var_kernels.h"
#include "gp_pred_kernels.h"   // PRED_LDS_MAX, PRED_MAXG: what ensure_tinv's product has to fit
#include "elbo_launch_plan.h"

// ------------------------------------------------------------------------------------------
// template dispatch on the padded dimension DT
// ------------------------------------------------------------------------------------------
// the padded dimensions DT the DT-templated kernels are instantiated for: one list for pick_dt and DISPATCH_DT (X(n, what the caller passes on))
#define VBMC_DT_LIST(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__) X(7, __VA_ARGS__) X(8, __VA_ARGS__) X(9, __VA_ARGS__) X(10, __VA_ARGS__) \
  X(11, __VA_ARGS__) X(12, __VA_ARGS__) X(14, __VA_ARGS__) X(16, __VA_ARGS__) X(18, __VA_ARGS__) X(20, __VA_ARGS__) X(24, __VA_ARGS__) X(28, __VA_ARGS__) X(32, __VA_ARGS__)
static int pick_dt(int D) {
#define X(n, ...) n,
  static const int dts[] = {VBMC_DT_LIST(X, 0)};
#undef X
  for (int t : dts)
    if (t >= D) return t;
  return -1;
}

#define DISPATCH_DT_CASE(n, ...) case n: { constexpr int DT = n; __VA_ARGS__; } break;
#define DISPATCH_DT(DTV, ...)                                                            \
  switch (DTV) {                                                                         \
    VBMC_DT_LIST(DISPATCH_DT_CASE, __VA_ARGS__)                                          \
    default: return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", dm.D);  \
  }

// the VALU entropy kernel: its LDS attribute (beyond 64 KiB only), then the launch
template <int DT, bool GRAD>
static hipError_t launch_entropy(dim3 grid, size_t lds, hipStream_t st, const EntArgs& ea) {
  hipError_t e = lds <= 64 * 1024 ? hipSuccess : hipFuncSetAttribute((const void*)k_entropy<DT, GRAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) hipLaunchKernelGGL((k_entropy<DT, GRAD>), grid, dim3(WAVE), lds, st, ea);
  return e;
}

// ---- MFMA entropy kernel dispatch: QS = ceil((D+2)/4) in 1..9 (one translation unit each, ent_mfma_inst.hip), KT = ceil(K/16) in 1..8
// (1..4 for QS > 6: register budget) -- and the lane-per-sample entropy kernel (entropy_lane.h; round 6): small mixtures, K <= 16 and D <= 12,
// one translation unit per padded dimension DT = 2, 4, .., 12 (ent_lane_inst.hip), KP = K rounded up to even.
// The per-instantiation launchers and occupancy queries, and the tables over them, from one list each (vbmc_amd/build.py: QS_RANGE, LANE_DT).
#define VBMC_QS_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)
#define VBMC_LANE_DT_LIST(X) X(2) X(4) X(6) X(8) X(10) X(12)
extern "C" {
#define X(n) int vbmc_launch_ent_mfma_qs##n(int, int, int, unsigned, unsigned, unsigned, void*, const EntArgs*); int vbmc_occupancy_ent_mfma_qs##n(int, int, int, const EntArgs*);
VBMC_QS_LIST(X)
#undef X
#define X(n) int vbmc_launch_ent_lane_dt##n(int, int, unsigned, unsigned, unsigned, void*, const EntArgs*); int vbmc_occupancy_ent_lane_dt##n(int, int, const EntArgs*);
VBMC_LANE_DT_LIST(X)
#undef X
}
#define X(n) {vbmc_launch_ent_mfma_qs##n, vbmc_occupancy_ent_mfma_qs##n},
static const struct { decltype(&vbmc_launch_ent_mfma_qs1) launch; decltype(&vbmc_occupancy_ent_mfma_qs1) occupancy; } ent_mfma_inst[9] = {VBMC_QS_LIST(X)};
#undef X
#define X(n) {vbmc_launch_ent_lane_dt##n, vbmc_occupancy_ent_lane_dt##n},
static const struct { decltype(&vbmc_launch_ent_lane_dt2) launch; decltype(&vbmc_occupancy_ent_lane_dt2) occupancy; } ent_lane_inst[6] = {VBMC_LANE_DT_LIST(X)};
#undef X

static int entropy_lane_occupancy(int D, int K, bool grad) {
  static int cache[6][9][2];      // 0: not asked yet
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  int& c = cache[(D + 1) / 2 - 1][(K + 1) / 2][grad ? 1 : 0];
  if (c == 0) { EntArgs q{}; const int nb = ent_lane_inst[(D + 1) / 2 - 1].occupancy(2 * ((K + 1) / 2), grad ? 1 : 0, &q); c = nb > 0 ? nb : -1; }
  return c;
}
// workgroups of the chosen instantiation per compute unit (registers and LDS: hipOccupancyMaxActiveBlocksPerMultiprocessor), cached
static int entropy_mfma_occupancy(int qs, int kt, int hv, bool grad, const EntArgs& ea) {
  if (qs < 1 || qs > 9) return -1;
  struct Key { int qs, kt, hv, grad, co, sparse, ldsk; };
  static std::vector<std::pair<Key, int>> cache;
  static std::mutex mu;                           // contexts of several host threads share the table
  std::lock_guard<std::mutex> lock(mu);
  const Key k{qs, kt, hv, grad ? 1 : 0, ea.lj.rows > 0 ? 1 : 0, ea.cutoff > 0.0 ? 1 : 0, ea.K * (ea.D + ENTP_EXTRA)};
  for (const auto& c : cache)
    if (!memcmp(&c.first, &k, sizeof(Key))) return c.second;
  const int nb = ent_mfma_inst[qs - 1].occupancy(kt, grad ? 1 : 0, hv, &ea);
  cache.push_back({k, nb});
  return nb;
}

// ------------------------------------------------------------------------------------------
// copy, pack and scatter kernels
// ------------------------------------------------------------------------------------------
// Small transfers between the pinned staging block and device memory by a kernel instead of the copy engines: the pinned block
// (hipHostMalloc: mapped into the device's address space, coherent) is read / written by the kernel directly over the host link.
// A DMA-engine copy between two kernels of a stream costs 50-100 us of hand-over latency each way (measured: 190-215 us between
// k_finalize of one batch and k_prep of the next at the headline shape, where the copies themselves are 0.3 MB); a kernel
// launch costs ~10 us.  Larger transfers use the copy engines.
#define COPY_KERNEL_MAX_BYTES ((size_t)4 << 20)
__global__ void k_copy_f64(size_t n, const double* __restrict__ src, double* __restrict__ dst) {
  VB_SMALL_PRIO();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// rows of `width` doubles, row r at src + r * stride -> dst + r * stride (same stride on both sides)
__global__ void k_copy_rows_f64(int rows, size_t stride, size_t width, const double* __restrict__ src, double* __restrict__ dst) {
  VB_SMALL_PRIO();
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < width; i += (size_t)gridDim.x * blockDim.x)
      dst[(size_t)r * stride + i] = src[(size_t)r * stride + i];
}
// separate_K outputs straight into the caller's layouts, written to the pinned block by the kernel: I_sk (S x K x R, s fastest)
// from the log-joint records, J_sjk (S x K x K x R) from the variance matrices (diagonal approximation: only J_kk is set,
// gplogjoint.m:283).  Replaces two pageable D2H copies and a host-side transposition (~0.15 ms of a 0.34 ms eval_fullelcbo).
__global__ void k_pack_sepk(int R, int S, int K, int LJS, int diag_only, const double* __restrict__ lj, const double* __restrict__ J,
                            double* __restrict__ hI, double* __restrict__ hJ) {
  const size_t nI = (size_t)R * S * K, nJ = J ? (size_t)R * S * K * K : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nI + nJ; i += (size_t)gridDim.x * blockDim.x) {
    if (i < nI) {
      const int s = (int)(i % S), k = (int)((i / S) % K), r = (int)(i / ((size_t)S * K));
      hI[i] = lj[(((size_t)r * S + s) * K + k) * LJS];
    } else {
      const size_t q = i - nI;
      const int s = (int)(q % S), j = (int)((q / S) % K), k = (int)((q / ((size_t)S * K)) % K), r = (int)(q / ((size_t)S * K * K));
      hJ[q] = (diag_only && j != k) ? 0.0 : J[(((size_t)r * S + s) * K + k) * K + j];
    }
  }
}

static bool copy_by_kernel(size_t bytes) { return bytes <= COPY_KERNEL_MAX_BYTES; }
// n doubles between the pinned block and device memory in stream st: k_copy_f64 while they are few (a failed launch shows at the
// caller's next hipGetLastError), the copy engine (`kind`) beyond
static hipError_t copy_f64_small(vbmc_ctx* ctx, hipStream_t st, double* dst, const double* src, size_t n, hipMemcpyKind kind) {
  (void)ctx;
  if (!copy_by_kernel(n * 8)) return hipMemcpyAsync(dst, src, n * 8, kind, st);
  hipLaunchKernelGGL(k_copy_f64, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, st, n, src, dst);
  return hipSuccess;
}

// gathered blocks of a sharded evaluation (ShardSpec below) -> the unsharded record layouts lj[r][s][k][LJS] and part[r][j][c][ncol]
__global__ void __launch_bounds__(256) k_shard_scatter(int R, int S, int K, int LJS, int C, int ncol, int world, int perS, int perC,
                                                       size_t blk, size_t ljn, const double* __restrict__ g,
                                                       double* __restrict__ lj, double* __restrict__ part) {
  const size_t nlj = (size_t)R * S * K * LJS, npe = part ? (size_t)R * K * C * ncol : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nlj + npe; i += (size_t)gridDim.x * blockDim.x) {
    if (i < nlj) {
      const int col = (int)(i % LJS);
      size_t t = i / LJS;
      const int k = (int)(t % K); t /= K;
      const int sidx = (int)(t % S), r = (int)(t / S);
      const int gk = sidx / perS, sl = sidx - gk * perS;
      lj[i] = g[(size_t)gk * blk + (((size_t)r * perS + sl) * K + k) * LJS + col];
    } else {
      const size_t e = i - nlj;
      const int col = (int)(e % ncol);
      size_t t = e / ncol;
      const int c = (int)(t % C); t /= C;
      const int j = (int)(t % K), r = (int)(t / K);
      const int gk = c / perC, cl = c - gk * perC;
      part[e] = g[(size_t)gk * blk + ljn + (((size_t)r * K + j) * perC + cl) * ncol + col];
    }
  }
}

// inv(L') of the Lchol samples, once per surrogate (gplite_pred's triangular product and the full-variance path use it); null when
// the solves no longer run 16 columns wide (N > 1136) or a 16-row tile of it does not fit the prediction kernel's LDS (N > 1248): those
// paths fall back to substitutions
static vbmc_status ensure_tinv(vbmc_ctx* ctx, const vbmc_gp* gp, bool* have) {
  const int N = gp->N, S = gp->S;
  const int Np = ((N + 15) >> 4) << 4, nblk = Np >> 4;
  *have = false;
  if (!gp->hasL || (size_t)16 * Np * 8 > PRED_LDS_MAX || nblk > PRED_MAXG || trsm_cw_for(N) != 16) return VBMC_OK;
  if (!gp->d_tinv) {
    const size_t bytes = (size_t)S * N * N * 8;
    TmpBuf pooled;            // a pooled surrogate's block: back to the pool unless the surrogate takes it over below
    double* t = nullptr;
    HIP_TRY(ctx, gp->pooled ? pooled.alloc(ctx, bytes) : hipMalloc((void**)&t, bytes));
    if (gp->pooled) t = pooled.as<double>();
    hipError_t e_ = tri_inverse_launch(ctx->stream, N, S, gp->L, gp->d_finv, gp->d_lchol, t, 0);
    if (e_ != hipSuccess) {
      if (!gp->pooled) (void)hipFree(t);
      return set_err(ctx, VBMC_ERR_HIP, "inv(L') failed: %s", hipGetErrorString(e_));
    }
    gp->d_tinv = t;
    (void)pooled.release();
  }
  *have = true;
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// the plan
// ------------------------------------------------------------------------------------------
// Everything one evaluation pass needs, resolved once: dims, device pointers, launch geometry.
// Its LaunchShape part is what the launch decisions are made from, its LaunchChoice part their outcome (elbo_launch_plan.h).
struct ElboPlan : LaunchShape, LaunchChoice {
  int compute_var = 0, var_stride = 0, ncol = 1, no_jacobian = 0;
  double beta = 0.0;
  bool mc = false, has_bnd = false, vgrad = false, any_nochol = false, needX = false, fin_big = false, tri_gemm = false;
  double *d_finbig = nullptr, *d_gamma = nullptr;
  double* d_dvs = nullptr;   // per-hyper-sample variance gradient block (dvarG_s), pooled for the call
  int r0 = 0;                // device-RNG key of restart r: r0 + r * rstride (vbmc_elbo_args.restart_offset / restart_stride)
  size_t n_theta = 0, n_up = 0, out_n = 0, ent_lds = 0, tlds = 0, n_sepk = 0;
  double *d_theta = nullptr, *d_fix = nullptr, *d_delta2 = nullptr, *d_bnd = nullptr;
  double *d_ljbar = nullptr;
  double *d_vpd = nullptr, *d_entp = nullptr, *d_lj = nullptr, *d_out = nullptr, *d_part = nullptr, *d_red = nullptr;
  double *d_Z = nullptr, *d_X = nullptr, *d_J = nullptr, *d_vg = nullptr, *d_var = nullptr, *d_vs = nullptr;   // d_vs: per-sample gradient vectors (k_var_sample)
  const double* d_eps = nullptr;
  double* out_direct = nullptr;   // the pinned result block itself: the finalize kernel writes the records there (small pipelined passes)
  long long eps_stride_r = 0;
  double TolCon = 0.0, WeightThreshold = 0.0, WeightPenalty = 0.0;
};

// the plan of a pass in a pipeline slot (abi_elbo_slots.hip) and the pinned block its results land in; vbmc_ctx.slot_plan points at one
struct SlotPlan { ElboPlan P; double* hout = nullptr; };

// ---- the size rules the plan and the launches share
// doubles of one log-joint record: I_k, w_k dmu[D], w_k dsigma, w_k dlambda[D] (elbo_kernels.h: k_logjoint)
static inline int lj_stride(int D) { return 2 * D + 2; }
// length of each of the three bounds vectors lb | ub | 1 / ell^2: mu (when optimised), sigma x lambda (when either is), eta (when optimised)
static inline int bounds_len(const ElboDims& dm) {
  return (dm.opt[0] ? dm.D * dm.K : 0) + ((dm.opt[1] || dm.opt[2]) ? dm.D * dm.K : 0) + (dm.opt[3] ? dm.K : 0);
}
// dynamic LDS of k_prep (prep_body: D K + 3 K + D doubles + one per wave)
static inline size_t prep_lds(const ElboDims& dm) { return ((size_t)dm.D * dm.K + 3 * dm.K + dm.D + 8) * sizeof(double); }
// threads of k_ent_reduce / k_reduce_both: one per column of a partial record, up to 256
static inline int reduce_threads(int ncol) { return ncol >= 192 ? 256 : (ncol >= 96 ? 128 : 64); }
// dynamic LDS of k_var_final: reduction scratch, two S-vectors, five T-vectors (only with a gradient), two K-vectors
#define VAR_FINAL_LDS(S_, K_, Tg_) ((VARFIN_THREADS + 2 * (size_t)(S_) + 5 * (size_t)(Tg_) + 2 * (size_t)(K_) + 8) * sizeof(double))
// k_finalize_ws keeps its reduction scratch, three K-vectors and -- unless they live in a global scratch block (`big`: where this
// exceeds 160 KB, 4 D K + 9 K > 19400, e.g. D = 32 with K > 141) -- the D x K soft-bound table and three T-vectors in LDS
static inline size_t fin_base_lds(const ElboDims& dm, bool big) { return (FIN_THREADS + 3 * (size_t)dm.K + (big ? 0 : (size_t)dm.D * dm.K + 3 * (size_t)dm.T) + 8) * sizeof(double); }
// What the finalize kernel stages in LDS on top of that, while the total stays within 96 KB: bit 1 (value 2) the restart's vp block and
// bounds, bit 0 its log-joint and entropy records.  Returns the launch's dynamic LDS.
static inline size_t fin_launch_lds(const ElboPlan& P, int* stage) {
  const ElboDims& dm = P.dm;
  size_t lds = fin_base_lds(dm, P.fin_big);
  const size_t stage_rec = ((size_t)dm.K * lj_stride(dm.D) + (P.mc ? (size_t)dm.K * P.ncol : 0)) * sizeof(double);
  const size_t stage_vp = ((size_t)VpLayout{dm.D, dm.K}.stride() + (P.has_bnd ? 3 * (size_t)bounds_len(dm) : 0)) * sizeof(double);
  *stage = 0;
  if (lds + stage_vp <= 96 * 1024) { *stage |= 2; lds += stage_vp; }
  if (lds + stage_rec <= 96 * 1024) { *stage |= 1; lds += stage_rec; }
  return lds;
}

// Validation (reference error ids), one H2D of theta | fixed vp | delta^2 | bounds, scratch sizing.
static vbmc_status elbo_plan(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* a, ElboPlan& P, int chunk_world = 0, bool pipelined = false) {
  if (!gp || !a) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_batch: null gp/args");
  if (a->struct_size != sizeof(vbmc_elbo_args))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_elbo_args.struct_size %u != %zu (ABI mismatch)", a->struct_size, sizeof(vbmc_elbo_args));
  ElboDims& dm = P.dm;
  dm.D = a->D; dm.K = a->K; dm.R = a->R; dm.S = gp->S; dm.N = gp->N;
  if (dm.D != gp->D) return set_err(ctx, VBMC_ERR_INVALID, "vp.D = %d but gp has D = %d", dm.D, gp->D);
  if (dm.K <= 0 || dm.R <= 0) return set_err(ctx, VBMC_ERR_INVALID, "K and R must be positive");
  if (dm.K > VBMC_LIM_K) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "K = %d > %d not accelerated", dm.K, VBMC_LIM_K);
  const int D = dm.D, K = dm.K, R = dm.R, S = dm.S;
  int T = 0;
  for (int g = 0; g < 4; ++g) dm.opt[g] = a->optimize[g] ? 1 : 0;
  dm.off_mu = dm.off_sigma = dm.off_lambda = dm.off_eta = -1;
  if (dm.opt[0]) { dm.off_mu = T; T += D * K; }
  if (dm.opt[1]) { dm.off_sigma = T; T += K; }
  if (dm.opt[2]) { dm.off_lambda = T; T += D; }
  if (dm.opt[3]) { dm.off_eta = T; T += K; }
  dm.T = T;
  if (T > 0 && !a->theta) return set_err(ctx, VBMC_ERR_INVALID, "theta is null");
  if ((!dm.opt[0] && !a->vp_mu) || (!dm.opt[1] && !a->vp_sigma) || (!dm.opt[2] && !a->vp_lambda) || (!dm.opt[3] && !a->vp_w))
    return set_err(ctx, VBMC_ERR_INVALID, "a vp field is required for every group that is not optimised");
  const int compute_grad = P.compute_grad = a->compute_grad ? 1 : 0;
  const int compute_var = P.compute_var = a->compute_var;
  if (compute_var < 0 || compute_var > 2) return set_err(ctx, VBMC_ERR_INVALID, "compute_var must be 0, 1 or 2");
  // negelcbo_vbmc.m:21-24
  if (compute_grad && a->beta != 0.0 && compute_var != 2)
    return set_err(ctx, VBMC_ERR_INVALID, "negelcbo_vbmc:vargrad Computation of the gradient of ELBO with full variance not supported.");
  // gplogjoint.m:29-32 (negelcbo requests dvarG whenever compute_var && compute_grad)
  if (compute_grad && compute_var == 1)
    return set_err(ctx, VBMC_ERR_INVALID, "gplogjoint:FullVarianceGradient gradient of the log joint variance needs compute_var == 2");
  if (a->separate_K && compute_grad)  // negelcbo_vbmc.m:57-59
    return set_err(ctx, VBMC_ERR_INVALID, "Computing the gradient of variational parameters and requesting per-component results at the same time.");
  if (compute_var != 0 && !gp->hasL)
    return set_err(ctx, VBMC_ERR_INVALID, "compute_var != 0 needs gp.post(s).L: upload the GP with L");
  if (compute_var != 0 && VAR_FINAL_LDS(S, K, compute_grad ? T : 0) > 160 * 1024)   // k_var_final: five T-vectors in LDS
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "variance gradient with %d variational parameters (> 4000) not accelerated", T);
  if (compute_var != 0 && trsm_cw_for(dm.N) == 0)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "variance path with N = %d > %d not accelerated", dm.N, trsm_max_n());
  P.beta = (std::isfinite(a->beta)) ? a->beta : 0.0;  // negelcbo_vbmc.m:15: non-finite beta -> 0
  // theta must be finite (the device exp does not propagate NaN)
  for (size_t i = 0; i < (size_t)T * R; ++i)
    if (!std::isfinite(a->theta[i])) return set_err(ctx, VBMC_ERR_INVALID, "theta contains a non-finite value at linear index %zu", i);

  int M = a->Ns;
  if (M < 0) return set_err(ctx, VBMC_ERR_INVALID, "Ns must be >= 0");
  if (a->restart_offset < 0 || a->restart_stride < 0) return set_err(ctx, VBMC_ERR_INVALID, "restart_offset / restart_stride must be >= 0");
  if (a->no_jacobian && compute_grad && a->bnd_lb)
    return set_err(ctx, VBMC_ERR_INVALID, "no_jacobian (JACOBIAN_FLAG = 0) is a form of the stand-alone functions: no soft bounds");
  if (a->dvarG && !(compute_grad && compute_var == 2)) return set_err(ctx, VBMC_ERR_INVALID, "dvarG needs compute_grad with compute_var = 2");
  if (a->dG_s && !compute_grad) return set_err(ctx, VBMC_ERR_INVALID, "dG_s (per-hyper-sample gradients) needs compute_grad");
  if (a->dvarG_s && !(compute_grad && compute_var == 2)) return set_err(ctx, VBMC_ERR_INVALID, "dvarG_s (per-hyper-sample variance gradients) needs compute_grad with compute_var = 2");
  if (a->plan_restarts < 0 || (a->plan_restarts > 0 && a->plan_restarts < R)) return set_err(ctx, VBMC_ERR_INVALID, "plan_restarts must be 0 or the size (>= R) of the batch this call is a share of");
  P.Rp = a->plan_restarts > 0 ? a->plan_restarts : R;
  P.no_jacobian = a->no_jacobian && compute_grad ? 1 : 0;
  P.r0 = a->restart_offset; P.rstride = a->restart_stride > 0 ? a->restart_stride : 1;
  M = ((M + 1) / 2) * 2;  // entmc_vbmc.m:45
  const int Mh = P.Mh = M / 2;
  P.mc = M > 0;
  if (P.mc && a->eps_mode != 0 && !a->eps) return set_err(ctx, VBMC_ERR_INVALID, "eps_mode %d needs eps", a->eps_mode);
  if (a->eps_mode < 0 || a->eps_mode > 2) return set_err(ctx, VBMC_ERR_INVALID, "eps_mode must be 0, 1 or 2");
  P.dt = pick_dt(D);
  if (P.dt < 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", D);
  // (here, with the other output checks that need no device: nothing has been enqueued yet)
  if (a->varG_s && !compute_var) return set_err(ctx, VBMC_ERR_INVALID, "varG_s needs compute_var != 0");
  P.fin_big = fin_base_lds(dm, false) > 160 * 1024;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  // ---- uploads: theta, fixed vp, delta^2, bounds (one pinned staging buffer, one H2D)
  const size_t n_theta = P.n_theta = (size_t)T * R;
  const size_t n_fix = (size_t)D * K + 2 * K + D;
  const size_t n_delta = D;
  const int Text = bounds_len(dm);
  P.has_bnd = a->bnd_lb != nullptr && a->bnd_ub != nullptr;
  const size_t n_bnd = P.has_bnd ? 3 * (size_t)Text : 0;     // lb | ub | 1 / ((ub - lb) TolCon)^2  (round 5: the reciprocals from the host)
  const size_t n_up = P.n_up = n_theta + n_fix + n_delta + n_bnd;
  P.out_n = (size_t)R * (OUT_HDR + 3 * T);
  // pinned block: staged inputs | result records | (separate_K) I_sk and J_sjk in the caller's layouts, when they are small enough
  // to be packed by a kernel (k_pack_sepk)
  P.n_sepk = (a->separate_K && (a->I_sk || a->J_sjk)) ? (size_t)S * K * R * (1 + (size_t)K) : 0;
  if (P.n_sepk * sizeof(double) > COPY_KERNEL_MAX_BYTES * 4) P.n_sepk = 0;
  VB_TRY(ensure_pin(ctx, (n_up + P.out_n + (size_t)S * K * R + P.n_sepk) * sizeof(double)));
  VB_TRY(ensure(ctx, ctx->theta, n_up * sizeof(double)));
  double* hp = (double*)ctx->pin;
  if (n_theta) memcpy(hp, a->theta, n_theta * sizeof(double));
  double* hfix = hp + n_theta;
  for (size_t i = 0; i < n_fix; ++i) hfix[i] = 1.0;
  if (a->vp_mu) memcpy(hfix, a->vp_mu, (size_t)D * K * sizeof(double));
  if (a->vp_sigma) memcpy(hfix + D * K, a->vp_sigma, K * sizeof(double));
  if (a->vp_lambda) memcpy(hfix + D * K + K, a->vp_lambda, D * sizeof(double));
  if (a->vp_w) memcpy(hfix + D * K + K + D, a->vp_w, K * sizeof(double));
  double* hdel = hfix + n_fix;
  for (int d = 0; d < D; ++d) hdel[d] = a->vp_delta ? a->vp_delta[d] * a->vp_delta[d] : 0.0;
  if (P.has_bnd) {
    memcpy(hdel + n_delta, a->bnd_lb, Text * sizeof(double));
    memcpy(hdel + n_delta + Text, a->bnd_ub, Text * sizeof(double));
    // softbndloss.m's ell = (UB - LB) TolCon enters as 1 / ell^2: (x - LB) / ell^2 and ((LB - x) / ell)^2 = (LB - x)^2 / ell^2 -- two fp64
    // divisions per bounded element in k_finalize_ws otherwise (44 division sequences, the longest of its tasks)
    double* hinv = hdel + n_delta + 2 * (size_t)Text;
    for (int i = 0; i < Text; ++i) { const double ell = (a->bnd_ub[i] - a->bnd_lb[i]) * a->TolCon; hinv[i] = 1.0 / (ell * ell); }
  }
  P.d_theta = (double*)ctx->theta.p;
  P.d_fix = P.d_theta + n_theta;
  P.d_delta2 = P.d_fix + n_fix;
  P.d_bnd = P.has_bnd ? P.d_delta2 + n_delta : nullptr;
  // (upload + unpacking in one launch and the reductions folded into the finalize kernel were built and measured in round 5: the host's
  // submit 23.6 -> 17.1 us at BASELINE configs[1], the step unchanged -- docs/history.md)
  if (copy_by_kernel(n_up * sizeof(double))) {
    hipLaunchKernelGGL(k_copy_f64, dim3((unsigned)std::min<size_t>((n_up + 255) / 256, 1024)), dim3(256), 0, st, n_up, (const double*)hp, P.d_theta);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(P.d_theta, hp, n_up * sizeof(double), hipMemcpyHostToDevice, st));
  }
  P.TolCon = a->TolCon; P.WeightThreshold = a->WeightThreshold; P.WeightPenalty = a->WeightPenalty;
  P.cutoff = a->sparse_cutoff > 0.0 ? a->sparse_cutoff : 0.0;

  // ---- scratch
  VB_TRY(ensure(ctx, ctx->prep, (size_t)R * VpLayout{D, K}.stride() * sizeof(double)));
  VB_TRY(ensure(ctx, ctx->entp, (size_t)R * K * (D + ENTP_EXTRA) * sizeof(double)));
  const int LJS = lj_stride(D);
  // (also set when the caller asks for the numbers a SHARDED evaluation gives -- chunk_world: the sharded path adds the log-joint
  // records per hyper-sample, so the unsharded evaluation it is compared with bit for bit must too)
  P.lj_records = a->separate_K || a->G_s || a->varG_s || a->dG_s || compute_var != 0 || chunk_world > 0 || a->chunk_world > 1;
  // (LJ_CO_SPLIT records per hyper-sample where the log joint may run as a role of the entropy launch: small grids only)
  const size_t ljrec = (size_t)R * S * K * LJS * ((lj_records_split(S, R, P.Rp, ctx->num_cu) && !P.lj_records) ? LJ_CO_SPLIT : 1);
  VB_TRY(ensure(ctx, ctx->ljpart, (ljrec + (size_t)R * K * LJS) * sizeof(double)));
  VB_TRY(ensure(ctx, ctx->out, P.out_n * sizeof(double)));
  const size_t nbig = P.fin_big ? (size_t)R * (3 * (size_t)T + (size_t)D * K) : 0;
  const size_t ngam = (!(a->Ns > 0) && K > 128) ? (size_t)R * K * K : 0;      // entlb's K x K table beyond the LDS
  if (nbig + ngam) {
    VB_TRY(ensure(ctx, ctx->bnd, (nbig + ngam) * sizeof(double)));
    P.d_finbig = nbig ? (double*)ctx->bnd.p : nullptr;
    P.d_gamma = ngam ? (double*)ctx->bnd.p + nbig : nullptr;
  }
  P.d_vpd = (double*)ctx->prep.p;
  P.d_entp = (double*)ctx->entp.p;
  P.d_lj = (double*)ctx->ljpart.p;
  P.d_ljbar = P.d_lj + ljrec;
  P.d_out = (double*)ctx->out.p;

  // ---- every launch decision of the pass (elbo_launch_plan.h); `sharded`: chunk_world > 0, the calls enqueued with ShardSpec.mode != 0
  // (NOT a->chunk_world > 1: that call gives a sharded evaluation's numbers from one unsharded pass)
  P.plan_restarts = a->plan_restarts; P.eps_mode = a->eps_mode; P.pipelined = pipelined;
  P.cw = chunk_world > 0 ? chunk_world : (a->chunk_world > 1 ? a->chunk_world : 1);   // sharded over cw devices
  const LaunchDevice dev{ctx->num_cu, ctx->prof_alone, ctx, entropy_mfma_occupancy, entropy_lane_occupancy};
  if (!plan_launch(P, dev, chunk_world > 0, read_launch_switches(), P))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "K = %d, D = %d: the eight-wave entropy kernel needs more than the 160 KiB of LDS", K, D);
  if (P.mc) {
    P.ncol = compute_grad ? (2 + 2 * D + K) : 1;
    VB_TRY(ensure(ctx, ctx->entpart, ((size_t)R * K * P.C * P.ncol + (size_t)R * K * P.ncol) * sizeof(double)));
    P.d_part = (double*)ctx->entpart.p;
    P.d_red = P.d_part + (size_t)R * K * P.C * P.ncol;
    const size_t eps_block = (size_t)D * Mh * K;
    if (a->eps_mode == 1) {
      const size_t n_eps = eps_block * (a->eps_shared ? 1 : (size_t)R);
      VB_TRY(ensure(ctx, ctx->eps, n_eps * sizeof(double)));
      HIP_TRY(ctx, hipMemcpyAsync(ctx->eps.p, a->eps, n_eps * sizeof(double), hipMemcpyHostToDevice, st));
      P.d_eps = (const double*)ctx->eps.p; P.eps_stride_r = a->eps_shared ? 0 : (long long)eps_block;
    } else if (a->eps_mode == 2) {
      P.d_eps = a->eps; P.eps_stride_r = a->eps_shared ? 0 : (long long)eps_block;
    }
    if (!P.use_mfma && !P.use_lane) {
      P.ent_lds = ((size_t)K * (P.dt + ENTP_EXTRA) + WAVE + (compute_grad ? (size_t)K * 65 : 0)) * sizeof(double);
      if (P.ent_lds > 160 * 1024) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "K = %d, D = %d needs %zu B of LDS (> 160 KiB)", K, D, P.ent_lds);
    }
  } else {
    const size_t ebs = 1 + (size_t)D * K + 2 * K + D;
    VB_TRY(ensure(ctx, ctx->entpart, (size_t)R * ebs * sizeof(double)));
    P.d_part = (double*)ctx->entpart.p;
  }
  if (compute_var != 0) {
    const int N = dm.N;
    P.var_stride = 2 + T;
    P.vgrad = compute_grad && compute_var == 2;
    bool any_chol = false;
    for (int s = 0; s < S; ++s) { P.any_nochol |= (gp->Lchol[s] == 0); any_chol |= (gp->Lchol[s] != 0); }
    const size_t nz = (size_t)R * S * K * N;
    VB_TRY(ensure(ctx, ctx->zbuf, nz * sizeof(double)));
    const size_t nJ = (size_t)R * S * K * K, nvg = (size_t)R * S * K * (2 * D + 1), nvo = (size_t)R * P.var_stride;
    // full variance without its gradient (eval_fullelcbo): V = inv(L') Z as a product with the explicit inverse (k_tri_gemm, out of
    // place into the X block) instead of the substitution
    if (compute_var == 1 && any_chol) VB_TRY(ensure_tinv(ctx, gp, &P.tri_gemm));
    P.needX = P.vgrad || P.any_nochol || P.tri_gemm;
    const size_t nvs = P.vgrad ? (size_t)R * S * 2 * (size_t)dm.T : 0;
    VB_TRY(ensure(ctx, ctx->varbuf, ((P.needX ? nz : 0) + nJ + nvg + nvo + nvs) * sizeof(double)));
    P.d_Z = (double*)ctx->zbuf.p;
    P.d_X = (double*)ctx->varbuf.p;
    P.d_J = P.d_X + (P.needX ? nz : 0);
    P.d_vg = P.d_J + nJ;
    P.d_var = P.d_vg + nvg;
    P.d_vs = P.d_var + nvo;
  }
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// the pass: its options, its stages and their driver
// ------------------------------------------------------------------------------------------
// cheap (no synchronisation) attribution of a failed launch to its kernel
#define LAUNCH_CHECK(ctx_, what)                                                                            \
  do {                                                                                                      \
    hipError_t le_ = hipGetLastError();                                                                     \
    if (le_ != hipSuccess) return set_err(ctx_, VBMC_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(le_)); \
  } while (0)

// Sharding of ONE evaluation over `world` ranks when there are fewer restarts than GPUs: rank g computes the
// expected-log-joint records of the hyper-samples [g perS, (g+1) perS) (misc/gplogjoint.m:98: the iterations over s are
// independent until the averaging at :399-413) and the entropy partial records of the sample chunks [g perC, (g+1) perC)
// -- with the SAME chunking the unsharded evaluation uses -- into one contiguous block; after the all-gather every rank
// scatters the blocks back into the unsharded layouts and runs the unsharded reductions + k_finalize, so the result is
// bit-identical to the 1-GPU evaluation by construction.
struct ShardSpec {
  int mode = 0;          // 0: unsharded; 1: begin (prep + own records -> send); 2: finish (prep + scatter + reductions + finalize)
  int rank = 0, world = 1;
  double* send = nullptr;            // mode 1: device block of shard_doubles(P, world)
  const double* gathered = nullptr;  // mode 2: device, world blocks in rank order
};
static inline int shard_per(int n, int world) { return (n + world - 1) / world; }
static inline size_t shard_lj_doubles(const ElboPlan& P, int world) { return (size_t)P.dm.R * shard_per(P.dm.S, world) * P.dm.K * lj_stride(P.dm.D); }
static inline size_t shard_ent_doubles(const ElboPlan& P, int world) { return P.mc ? (size_t)P.dm.R * P.dm.K * shard_per(P.C, world) * P.ncol : 0; }
static inline size_t shard_doubles(const ElboPlan& P, int world) { return shard_lj_doubles(P, world) + shard_ent_doubles(P, world); }
// The slice of the hyper-samples [s0, s0 + ns) and of the entropy chunks [c0, c0 + nc) a pass computes, and where its log-joint records
// go: a rank's share into its send block in mode 1, everything into the plan's own block otherwise.  perS / perC: slots per rank.
struct ShardSlice { int perS, s0, ns, perC, c0, nc; double* lj_out; };
static inline ShardSlice shard_slice(const ShardSpec& sh, const ElboPlan& P) {
  const bool own = sh.mode == 1;
  const int S = P.dm.S, C = P.C, perS = shard_per(S, sh.world), perC = shard_per(C, sh.world);
  const int s0 = own ? std::min(S, sh.rank * perS) : 0, c0 = own ? std::min(C, sh.rank * perC) : 0;
  return {perS, s0, own ? std::min(S, s0 + perS) - s0 : S, perC, c0, own ? std::min(C, c0 + perC) - c0 : C, own ? sh.send : P.d_lj};
}

// What one enqueue of a plan may ask for beyond the plan itself.  fuse / fuse_iter: this pass's finalize kernel applies the Adam update
// of iteration fuse_iter and unpacks the new theta for the NEXT pass, which is then enqueued with skip_prep (the on-device optimiser
// loop: one launch per iteration less, vbmc_adam_batch).
struct PassOpts {
  ShardSpec shard;
  const AdamState* fuse = nullptr; int fuse_iter = 0;
  bool skip_prep = false;
};

// One enqueue of a plan: what its stages share (st: the context's stream), and the stages
struct Pass {
  vbmc_ctx* ctx; const vbmc_gp* gp;
  const ElboPlan& P; const ElboDims& dm;
  const PassOpts& o; const ShardSpec& sh;
  hipStream_t st; unsigned long long seed;
  ShardSlice sl;
  vbmc_status prep() const, logjoint(hipStream_t ls) const, shard_scatter() const, entropy() const, entropy_reduce() const,
      entropy_bound() const, variance() const, finalize() const;
};

// theta -> vp fields + packed per-component parameters
inline vbmc_status Pass::prep() const {
  const size_t lds = prep_lds(dm);
  if (lds > 64 * 1024)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_prep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (!o.skip_prep) {
    hipLaunchKernelGGL(k_prep, dim3(dm.R), dim3(256), lds, st, dm, (const double*)P.d_theta, P.d_fix, P.d_vpd, P.d_entp);
    LAUNCH_CHECK(ctx, "k_prep");
  }
  return VBMC_OK;
}

// Expected log joint: enqueued on `ls` -- the context's stream, or the auxiliary one beside the entropy kernel -- unless it runs as a
// role of the entropy launch.  Which of these, and which kernel, is the plan's decision (elbo_launch_plan.h: plan_launch).
inline vbmc_status Pass::logjoint(hipStream_t ls) const {
  const int D = dm.D, K = dm.K, R = dm.R, S = dm.S;
  if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ls));
  if (!P.role() && sl.ns > 0) {
    const bool lj_mfma = P.lj_form == VBMC_LJFORM_MFMA_GRAD || P.lj_form == VBMC_LJFORM_MFMA_VALUE;
    ctx->last_lj_form = P.lj_form;
    DISPATCH_DT(P.dt, {
      const int nw = (K + 15) / 16;
      // the kernels reach hyper-sample s only through alpha + s N and gpc + s GPC_STRIDE and use dm.S as the record
      // stride: a slice [s0, s0 + ns) is the same launch with shifted pointers (the plan chose the variant from the FULL S,
      // so a sharded evaluation runs the kernel the unsharded one would)
      ElboDims dml = dm;
      dml.S = sh.mode == 1 ? sl.perS : S;
      const double* al = gp->alpha + (size_t)sl.s0 * dm.N;
      const double* gc = gp->gpc + (size_t)sl.s0 * GPC_STRIDE(D);
      if (lj_mfma) {
        // rows rho = r K + k of the whole batch, sixteen per wave, nw waves per workgroup (what one restart's K components take): a
        // workgroup is (hyper-sample, row group) and only the last group can hold padding.  R = 1: one group, the launch as it was.
        const int ngrp = ((R * K + 15) / 16 + nw - 1) / nw;
        const size_t mom_lds = LJ_MFMA_DYN_LDS(DT, nw);   // feature rows / moment exchange
        const auto kern = P.compute_grad ? k_logjoint_mfma<DT, true> : k_logjoint_mfma<DT, false>;
        hipLaunchKernelGGL(kern, dim3(sl.ns, ngrp), dim3(WAVE * nw), mom_lds, ls, dml, P.d_vpd, gp->X, gp->d_meanX, al, gc, P.d_delta2, sl.lj_out);
        LAUNCH_CHECK(ctx, "k_logjoint_mfma");
      } else {
        hipLaunchKernelGGL((k_logjoint<DT>), dim3((K + 3) / 4, sl.ns, R), dim3(P.lj_split ? WAVE * LJ_MAXW : WAVE), 0, ls, dml, P.d_vpd, gp->X, al, gc,
                           P.d_delta2, sl.lj_out, P.compute_grad);
        LAUNCH_CHECK(ctx, "k_logjoint");
      }
    });
  }
  if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ls));
  // log-joint partials summed over hyper-samples (in sample order), one record per (r, k); on the main stream of an MC
  // evaluation this shares a launch with the entropy reduction (entropy_reduce)
  if (sh.mode == 0 && (P.fork || !P.mc)) hipLaunchKernelGGL(k_lj_reduce, dim3(K, R), dim3(64), 0, ls, S, K, lj_stride(D), P.d_lj, P.d_ljbar);
  LAUNCH_CHECK(ctx, "k_lj_reduce");
  return VBMC_OK;
}

// shard mode 2: the gathered records of all ranks -> the unsharded layouts
inline vbmc_status Pass::shard_scatter() const {
  const int K = dm.K, R = dm.R, S = dm.S, LJS = lj_stride(dm.D);
  const size_t blk = shard_doubles(P, sh.world), ljn = shard_lj_doubles(P, sh.world);
  const size_t tot = (size_t)R * S * K * LJS + (P.mc ? (size_t)R * K * P.C * P.ncol : 0);
  hipLaunchKernelGGL(k_shard_scatter, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, st, R, S, K, LJS,
                     P.C, P.ncol, sh.world, sl.perS, sl.perC, blk, ljn, sh.gathered, P.d_lj, P.mc ? P.d_part : nullptr);
  LAUNCH_CHECK(ctx, "k_shard_scatter");
  if (!P.mc) hipLaunchKernelGGL(k_lj_reduce, dim3(K, R), dim3(64), 0, st, S, K, LJS, P.d_lj, P.d_ljbar);
  return VBMC_OK;
}

// Monte-Carlo entropy: the chunk partials of this pass's chunks (nothing in shard mode 2: they came with the gathered blocks)
inline vbmc_status Pass::entropy() const {
  const int D = dm.D, K = dm.K, R = dm.R, nc = sl.nc;
  const bool co = P.role();
  EntArgs ea{};
  ea.entp = P.d_entp; ea.vpd = P.d_vpd;
  // sharded: this rank's chunks [c0, c0 + nc) of the unsharded chunking, written to slots 0 .. nc-1 of a perC-slot record
  ea.part = sh.mode == 1 ? sh.send + shard_lj_doubles(P, sh.world) : P.d_part;
  ea.D = D; ea.K = K; ea.Mh = P.Mh; ea.C = sh.mode == 1 ? sl.perC : P.C; ea.c0 = sl.c0; ea.tiles_per_chunk = P.tpc; ea.ncol = P.ncol; ea.seed = seed;
  ea.eps = P.d_eps; ea.eps_stride_r = P.eps_stride_r; ea.cutoff = P.cutoff; ea.r0 = P.r0; ea.rstride = P.rstride;
  ea.prio = 1;   // progress-ordered wave priorities (entropy_mfma.h)
  ea.co_c1 = P.co_c1; ea.co_c2 = P.co_c2; ea.co_tpc2 = P.co_tpc2;
  const bool walk = P.walk_tpw > 0;      // (never with a role or a shard: plan_launch)
  if (walk) { ea.walk_tpw = P.walk_tpw; ea.walk_R = R; }
  if (co) {
    LjCo& lc = ea.lj;
    lc.nsplit = P.co_nsplit; lc.nwg = P.co_nwg; lc.rows = P.co_rows;
    lc.want_grad = P.compute_grad;
    lc.dm = dm; lc.X = gp->X; lc.alpha = gp->alpha; lc.gpc = gp->gpc; lc.delta2 = P.d_delta2; lc.lj = P.d_lj;
  }
  if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev[2], st));
  if (sh.mode != 2 && nc > 0) {
    ctx->last_ent_form = P.ent_form;
    if (co) ctx->last_lj_form = P.lj_form;
  }
  if (sh.mode == 2 || nc <= 0) {
  } else if (P.use_lane) {
    ea.nc_launch = nc;
    // workgroups per restart: four (component, chunk) items each -- and, where the launch carries the role, at least one wave per cell
    // group (a single chain has ten entropy waves and twenty-four cell groups: two groups behind each other on a wave were most of its launch)
    int gx = (K * nc + ENT_LANE_WAVES_HOST - 1) / ENT_LANE_WAVES_HOST;
    if (co) gx = std::max(gx, (ea.lj.nwg + ENT_LANE_WAVES_HOST - 1) / ENT_LANE_WAVES_HOST);
    if (ent_lane_inst[(D + 1) / 2 - 1].launch(2 * ((K + 1) / 2), P.compute_grad, gx, 1 + P.co_rows, R, (void*)st, &ea) != 0)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "no lane entropy kernel for D = %d, K = %d", D, K);
  } else if (P.use_mfma) {
    const dim3 g = walk ? dim3(P.walk_nw, 1, 1) : dim3((co && P.co_c2 > 0) ? P.co_c1 : nc, K + P.co_rows, R);
    if (P.qs < 1 || P.qs > 9 || ent_mfma_inst[P.qs - 1].launch(P.kt, P.compute_grad, P.hv, g.x, g.y, g.z, (void*)st, &ea) != 0)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "no MFMA entropy kernel for D = %d", D);
  } else {
    DISPATCH_DT(P.dt, {
      HIP_TRY(ctx, (P.compute_grad ? launch_entropy<DT, true>(dim3(nc, K, R), P.ent_lds, st, ea) : launch_entropy<DT, false>(dim3(nc, K, R), P.ent_lds, st, ea)));
    });
  }
  LAUNCH_CHECK(ctx, "the entropy kernel");
  if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev[3], st));
  return VBMC_OK;
}

// chunk partials -> one record per (r, j), summed in chunk order; where the log joint was not forked, its reduction rides along
inline vbmc_status Pass::entropy_reduce() const {
  if (P.fork)
    hipLaunchKernelGGL(k_ent_reduce, dim3(dm.K, dm.R), dim3(reduce_threads(P.ncol)), 0, st, P.C, P.ncol, P.d_part, P.d_red, P.walk_tpw, (P.Mh + 15) / 16);
  else
    hipLaunchKernelGGL(k_reduce_both, dim3(dm.K, dm.R, 2), dim3(reduce_threads(P.ncol)), 0, st, P.C, P.ncol,
                       P.d_part, P.d_red, P.role() ? dm.S * P.co_nsplit : dm.S, lj_stride(dm.D), P.d_lj, P.d_ljbar, P.walk_tpw, (P.Mh + 15) / 16);
  LAUNCH_CHECK(ctx, "k_ent_reduce / k_reduce_both");
  return VBMC_OK;
}

// Ns = 0: the deterministic lower bound of the entropy (ent/entlb_vbmc.m)
inline vbmc_status Pass::entropy_bound() const {
  const size_t lds = ((P.d_gamma ? 0 : (size_t)dm.K * dm.K) + dm.K + 256) * sizeof(double);
  if (lds > 64 * 1024)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_entlb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_entlb, dim3(dm.R), dim3(256), lds, st, dm, P.d_vpd, P.d_part, P.compute_grad, P.d_gamma);
  LAUNCH_CHECK(ctx, "k_entlb");
  ctx->last_ent_form = P.ent_form;
  return VBMC_OK;
}

// variance of the expected log joint (gplogjoint.m:273-337,375-413)
inline vbmc_status Pass::variance() const {
  const int K = dm.K, R = dm.R, S = dm.S, T = dm.T, N = dm.N;
  vbmc_var_launch_info& rec = ctx->last_var;   // vbmc_ctx_last_variance: filled as the kernels are enqueued, from what each launch reads
  rec = vbmc_var_launch_info{};
  rec.compute_var = P.compute_var; rec.symm = P.any_nochol ? 1 : 0; rec.tri_gemm = P.tri_gemm ? 1 : 0; rec.vgrad = P.vgrad ? 1 : 0;
  DISPATCH_DT(P.dt, {
    hipLaunchKernelGGL((k_var_z<DT>), dim3(K, S, R), dim3(WAVE), 0, st, dm, P.d_vpd, gp->X, gp->gpc, P.d_delta2, P.d_Z);
    LAUNCH_CHECK(ctx, "k_var_z");
  });
  if (P.any_nochol) hipLaunchKernelGGL(k_symm, dim3(32, S, R), dim3(256), 0, st, N, K, S, gp->L, gp->d_lchol, P.d_Z, P.d_X);
  LAUNCH_CHECK(ctx, "k_symm");
  if (P.tri_gemm) {
    hipLaunchKernelGGL(k_tri_gemm, dim3(((N + 15) / 16) * ((K + 15) / 16), S, R), dim3(64), 0, st, N, K, S, gp->d_tinv, gp->d_lchol, (const double*)P.d_Z, P.d_X);
    LAUNCH_CHECK(ctx, "k_tri_gemm");
  } else {
    HIP_TRY(ctx, trsm_fwd_launch(st, N, K, S, R, gp->L, gp->d_finv, gp->d_lchol, P.d_Z));
    trsm_form_for(N, &rec.fwd_solve, &rec.solve_width);
  }
  rec.gram = P.compute_var == 1 ? VBMC_VARGRAM_MFMA : VBMC_VARGRAM_WAVE;
  if (P.compute_var == 1)   // full K x K matrix: Gram products on the matrix cores, one workgroup per (s, r)
    hipLaunchKernelGGL(k_var_gram_mfma, dim3(S, R), dim3(1024), 0, st, dm, P.d_vpd, gp->gpc, P.d_delta2, gp->d_sn2, gp->d_lchol, P.d_Z, P.d_X, P.d_J, P.tri_gemm ? 1 : 0);
  else
    hipLaunchKernelGGL(k_var_gram, dim3(16, S, R), dim3(256), 0, st, dm, P.d_vpd, gp->gpc, P.d_delta2, gp->d_sn2, gp->d_lchol, P.d_Z, P.d_X, P.d_J, P.compute_var == 1 ? 1 : 0);
  LAUNCH_CHECK(ctx, "k_var_gram");
  if (P.vgrad) {
    HIP_TRY(ctx, trsm_bwd_launch(st, N, K, S, R, gp->L, gp->d_finv, gp->d_lchol, P.d_Z, P.d_X));
    trsm_form_for(N, &rec.bwd_solve, &rec.solve_width);
    DISPATCH_DT(P.dt, {
      hipLaunchKernelGGL((k_vargrad<DT>), dim3(K, S, R), dim3(WAVE), 0, st, dm, P.d_vpd, gp->X, gp->gpc, P.d_delta2, gp->d_sn2, gp->d_lchol, P.d_X, P.d_vg);
      LAUNCH_CHECK(ctx, "k_vargrad");
    });
  }
  VarFinArgs va{};
  va.dm = dm; va.vpd = P.d_vpd; va.gpc = gp->gpc; va.delta2 = P.d_delta2; va.lj = P.d_lj; va.J = P.d_J;
  va.vg = P.vgrad ? P.d_vg : nullptr; va.compute_var = P.compute_var; va.want_grad = P.compute_grad; va.stride = P.var_stride;
  va.out = P.d_var;
  va.no_jacobian = P.no_jacobian; va.dvs_out = P.d_dvs; va.vs = P.d_vs;
  if (P.vgrad) {
    const size_t slds = VAR_SAMPLE_LDS(K, T);
    if (slds > 64 * 1024)
      HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_var_sample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slds));
    hipLaunchKernelGGL(k_var_sample, dim3(S, R), dim3(VARSMP_THREADS), slds, st, va);
    rec.sample_lds = (int32_t)slds;
    LAUNCH_CHECK(ctx, "k_var_sample");
  }
  const size_t vlds = VAR_FINAL_LDS(S, K, P.compute_grad ? T : 0);
  if (vlds > 64 * 1024)
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_var_final, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vlds));
  hipLaunchKernelGGL(k_var_final, dim3(R), dim3(VARFIN_THREADS), vlds, st, va);
  rec.final_lds = (int32_t)vlds;
  LAUNCH_CHECK(ctx, "k_var_final");
  return VBMC_OK;
}

// The reduced records -> the packed results [F G H varG varGss | dF dG dH] per restart.  k_finalize_ws: the wave-specialised form (one
// barrier; round 3 -- the sequential kernel with its ~18 barriers is in the history); it carries the fused Adam update + unpacking of
// the next iteration.
inline vbmc_status Pass::finalize() const {
  FinArgs fa{};
  fa.dm = dm;
  if (P.mc) { fa.entpart = P.d_red; fa.M = P.Mh; fa.C = 1; fa.ncol = P.ncol; }
  else fa.entlb = P.d_part;
  fa.vpd = P.d_vpd; fa.theta = P.d_theta; fa.ljbar = P.d_ljbar; fa.var = P.d_var; fa.var_stride = P.d_var ? P.var_stride : 0;
  fa.bnd = P.d_bnd; fa.has_bnd = P.has_bnd ? 1 : 0;
  fa.TolCon = P.TolCon; fa.WeightThreshold = P.WeightThreshold; fa.WeightPenalty = P.WeightPenalty;
  fa.beta = P.beta; fa.want_grad = P.compute_grad; fa.out = P.out_direct ? P.out_direct : P.d_out; fa.no_jacobian = P.no_jacobian;
  fa.invS = 1.0 / P.dm.S; fa.invM = fa.M > 0 ? 1.0 / (2.0 * fa.M) : 0.0;
  fa.big = P.d_finbig;
  const size_t lds = fin_launch_lds(P, &fa.stage);
  if (o.fuse) {
    fa.next_iter = o.fuse_iter; fa.next_A = *o.fuse; fa.next_theta = P.d_theta; fa.next_vpfix = P.d_fix; fa.next_vpd = P.d_vpd; fa.next_entp = P.d_entp;
  }
  const auto kern = (fa.stage == 3 && !fa.big) ? k_finalize_ws<true> : k_finalize_ws<false>;
  if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(dm.R), dim3(FIN_THREADS), lds, st, fa);
  LAUNCH_CHECK(ctx, "k_finalize");
  return VBMC_OK;
}

// Enqueue one evaluation pass on the context's stream: reads theta from P.d_theta, leaves the packed
// results [F G H varG varGss | dF dG dH] per restart in P.d_out.  No host synchronisation.
static vbmc_status elbo_enqueue(vbmc_ctx* ctx, const vbmc_gp* gp, const ElboPlan& P, unsigned long long seed, const PassOpts& o = PassOpts{}) {
  const int mode = o.shard.mode;
  hipStream_t st = ctx->stream;
  const Pass ps{ctx, gp, P, P.dm, o, o.shard, st, seed, shard_slice(o.shard, P)};
  if (mode != 2) ctx->last_ent_form = ctx->last_lj_form = 0;   // vbmc_ctx_last_launch: set by the stages as the kernels are enqueued
  VB_TRY(ps.prep());
  if (P.fork) {                   // the log joint goes beside the entropy kernel, after it is queued (below)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
  } else if (mode != 2) {
    VB_TRY(ps.logjoint(st));
  }
  if (mode == 2) VB_TRY(ps.shard_scatter());
  if (P.mc) {
    VB_TRY(ps.entropy());
    if (mode == 1) return VBMC_OK;   // the records are in the send block; the exchange and the rest follow in mode 2
    VB_TRY(ps.entropy_reduce());
  } else {
    if (mode == 1) return VBMC_OK;   // the deterministic bound is O(K^2 D): every rank evaluates it in mode 2
    VB_TRY(ps.entropy_bound());
  }
  if (P.fork) {   // the entropy kernel is already queued on the main stream: the log joint fills in around it
    VB_TRY(ps.logjoint(ctx->aux));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
    HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
  }
  if (P.compute_var != 0) VB_TRY(ps.variance());
  VB_TRY(ps.finalize());
  HIP_TRY(ctx, hipGetLastError());
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// read-back and unpacking
// ------------------------------------------------------------------------------------------
// The packed read-back of an enqueued pass into pinned memory (no synchronisation) ...
static vbmc_status elbo_enqueue_readback(vbmc_ctx* ctx, const ElboPlan& P, const vbmc_elbo_args* a, double* hout) {
  const int R = P.dm.R, T = P.dm.T;
  // record per restart: [F G H varG varGss | dF (T) | dG (T) | dH (T)]; without dG / dH only the leading part moves
  const size_t OSr = OUT_HDR + 3 * (size_t)T;
  const bool lead = P.compute_grad && !a->dG && !a->dH && R > 1;
  const size_t width = OUT_HDR + (size_t)T;
  if (copy_by_kernel((lead ? (size_t)R * width : P.out_n) * sizeof(double))) {
    if (lead)
      hipLaunchKernelGGL(k_copy_rows_f64, dim3((unsigned)((width + 255) / 256), (unsigned)std::min(R, 1024)), dim3(256), 0, ctx->stream, R, OSr, width, (const double*)P.d_out, hout);
    else
      hipLaunchKernelGGL(k_copy_f64, dim3((unsigned)std::min<size_t>((P.out_n + 255) / 256, 1024)), dim3(256), 0, ctx->stream, P.out_n, (const double*)P.d_out, hout);
    HIP_TRY(ctx, hipGetLastError());
  } else if (lead) {
    HIP_TRY(ctx, hipMemcpy2DAsync(hout, OSr * sizeof(double), P.d_out, OSr * sizeof(double), width * sizeof(double), R, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(hout, P.d_out, P.out_n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  return VBMC_OK;
}

// ... and, once it has landed, its unpacking into the caller's arrays (restart q of the pass is column col0 + q * cstride there:
// 0, 1 for a batch of its own; g, G for the share of rank g of a batch dealt over G ranks)
static void elbo_unpack(const ElboPlan& P, const vbmc_elbo_args* a, const double* hout, int col0 = 0, int cstride = 1) {
  const int R = P.dm.R, T = P.dm.T;
  const size_t OS = OUT_HDR + 3 * (size_t)T;
  for (int q = 0; q < R; ++q) {
    const double* o = hout + (size_t)q * OS;
    const size_t r = (size_t)col0 + (size_t)q * cstride;
    if (a->F) a->F[r] = o[0];
    if (a->G) a->G[r] = o[1];
    if (a->H) a->H[r] = o[2];
    if (a->varG) a->varG[r] = o[3];
    if (a->varGss) a->varGss[r] = o[4];
    if (P.compute_grad) {
      if (a->dF) memcpy(a->dF + r * T, o + OUT_HDR, T * sizeof(double));
      if (a->dG) memcpy(a->dG + r * T, o + OUT_HDR + T, T * sizeof(double));
      if (a->dH) memcpy(a->dH + r * T, o + OUT_HDR + 2 * T, T * sizeof(double));
    }
  }
}

// One packed D2H of the results of an enqueued pass (+ I_sk / J_sjk / per-sample outputs when requested); synchronises.
static vbmc_status elbo_read_results(vbmc_ctx* ctx, const ElboPlan& P, const vbmc_elbo_args* a) {
  const ElboDims& dm = P.dm;
  const int K = dm.K, R = dm.R, S = dm.S, D = dm.D;
  const int LJS = lj_stride(D);
  hipStream_t st = ctx->stream;

  // ---- results: one packed D2H (+ I_sk / J_sjk when requested)
  double* hout = (double*)ctx->pin + P.n_up;
  VB_TRY(elbo_enqueue_readback(ctx, P, a, hout));
  std::vector<double> ljh, Jh;
  double* hI = hout + P.out_n + (size_t)S * K * R;   // (behind the slack the block has always carried)
  double* hJ = hI + (size_t)S * K * R;
  const bool packed = P.n_sepk != 0 && copy_by_kernel(0);
  const bool wantJ = a->separate_K && a->J_sjk && P.d_J;
  if (packed) {
    const size_t tot = (size_t)R * S * K * (1 + (wantJ ? (size_t)K : 0));
    hipLaunchKernelGGL(k_pack_sepk, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, R, S, K, LJS,
                       P.compute_var == 2 ? 1 : 0, (const double*)P.d_lj, wantJ ? (const double*)P.d_J : nullptr, hI, hJ);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    if (a->separate_K && a->I_sk) {
      ljh.resize((size_t)R * S * K * LJS);
      HIP_TRY(ctx, hipMemcpyAsync(ljh.data(), P.d_lj, ljh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (wantJ) {
      Jh.resize((size_t)R * S * K * K);
      HIP_TRY(ctx, hipMemcpyAsync(Jh.data(), P.d_J, Jh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
  }
  // the per-hyper-sample outputs pass through pooled blocks, held until this function returns
  std::vector<double> psh, dgsh;
  TmpBuf d_ps, d_dgs;
  if (a->G_s || a->varG_s) {   // gplogjoint's avg_flag = 0 outputs (varG_s without a variance: refused by elbo_plan)
    HIP_TRY(ctx, d_ps.alloc(ctx, 2 * (size_t)S * R * sizeof(double)));
    hipLaunchKernelGGL(k_per_sample, dim3((S + 63) / 64, R), dim3(64), 0, st, dm, P.d_vpd, P.d_lj, P.d_J, P.compute_var, d_ps.as<double>(),
                       a->varG_s ? d_ps.as<double>() + (size_t)S * R : nullptr);
    psh.resize(2 * (size_t)S * R);
    hipError_t e_ = hipMemcpyAsync(psh.data(), d_ps.p, psh.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e_ != hipSuccess) return set_err(ctx, VBMC_ERR_HIP, "per-sample read-back: %s", hipGetErrorString(e_));
  }
  if (a->dG_s) {               // gplogjoint's dF with avg_flag = 0: T x S per restart
    const size_t n = (size_t)dm.T * S * R;
    HIP_TRY(ctx, d_dgs.alloc(ctx, n * sizeof(double)));
    hipLaunchKernelGGL(k_per_sample_grad, dim3(S, R), dim3(256), 0, st, dm, P.d_vpd, P.d_lj, P.no_jacobian, d_dgs.as<double>());
    dgsh.resize(n);
    hipError_t e_ = hipMemcpyAsync(dgsh.data(), d_dgs.p, n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e_ != hipSuccess) return set_err(ctx, VBMC_ERR_HIP, "per-sample gradient read-back: %s", hipGetErrorString(e_));
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (es != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, VBMC_ERR_HIP, "vbmc_elbo_batch: %s", hipGetErrorString(es)); }
  if (a->dG_s) memcpy(a->dG_s, dgsh.data(), dgsh.size() * sizeof(double));
  if (a->G_s) memcpy(a->G_s, psh.data(), (size_t)S * R * sizeof(double));
  if (a->varG_s) memcpy(a->varG_s, psh.data() + (size_t)S * R, (size_t)S * R * sizeof(double));
  if (ctx->profiling) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->last_lj_ms = ms;
    if (P.mc && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->last_ent_ms = ms;
  }
  elbo_unpack(P, a, hout);
  if (a->dvarG && P.vgrad && P.d_var) {   // gplogjoint's dvarF: behind the two variance scalars of each restart's record
    HIP_TRY(ctx, hipMemcpy2DAsync(a->dvarG, (size_t)dm.T * sizeof(double), P.d_var + 2, (size_t)P.var_stride * sizeof(double),
                                  (size_t)dm.T * sizeof(double), R, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  if (packed) {
    if (a->I_sk) memcpy(a->I_sk, hI, (size_t)R * S * K * sizeof(double));
    if (wantJ) memcpy(a->J_sjk, hJ, (size_t)R * S * K * K * sizeof(double));
  } else if (a->separate_K && a->I_sk) {
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < K; ++k)
        for (int s = 0; s < S; ++s) a->I_sk[s + (size_t)S * (k + (size_t)K * r)] = ljh[(((size_t)r * S + s) * K + k) * LJS];
  }
  if (!Jh.empty()) {
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < K; ++k)
        for (int j = 0; j < K; ++j)
          for (int s = 0; s < S; ++s)
            a->J_sjk[s + (size_t)S * (j + (size_t)K * (k + (size_t)K * r))] =   // diagonal approximation: only J_kk is set (gplogjoint.m:283)
                (P.compute_var == 2 && j != k) ? 0.0 : Jh[(((size_t)r * S + s) * K + k) * K + j];
  }
  return VBMC_OK;
}

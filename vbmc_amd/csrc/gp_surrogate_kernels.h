// Sampling the GP surrogate on the device (misc/gpsample_vbmc.m -> gplite/gplite_sample.m, method 'parallel'): E ensembles of the
// library's indexed-uniform ensemble slice sampler (is_sample_kernels.h: k_is_step, unchanged) on the target
//   log_gpfun(x) = ybar - (ys2 - VarThresh) [ys2 >= VarThresh] - beta sqrt(ys2)                         (gplite_sample.m:109-117)
// with [ybar, ys2] the prediction of the noisy pair AVERAGED over all S hyper-samples (gplite_pred.m:154-164).  Ensembles and
// hyper-samples are decoupled: every candidate of every ensemble is evaluated under every hyper-sample.  One ROUND is
//   k_is_step     one workgroup per ensemble: consume, commit, record, propose (the sampler of the IMIQR importance sampler as it is)
//   k_gs_pred     grid (16-point tiles of an ensemble's candidates, E, S): the body of k_is_pred with the point buffer indexed by the
//                 ensemble and the GP quantities by the hyper-sample; ymu (= fmu: no ystar) and ys2 into [s][e][c]; no target
//   k_gs_target   one candidate per lane: the sums over s in index order (contraction off), the VarThresh / beta rule, a value that is
//                 not finite becomes -Inf; written where k_is_step reads the values
// The chain closes with
//   k_gs_finish   recorded walkers (Nm x D x E, transformed space) -> X (Ns x D): row r = e + E i is record i of ensemble e, rows >= Ns
//                 are dropped; with origflag the inverse transform and the clamp of vpt_finish, the functions k_vp_draw uses
// The noise estimate (gpsample_vbmc.m:30-38): Nnn unbalanced transformed-space draws of k_vp_draw, the nearest row of X_rescaled per
// draw by k_nn_noise (first minimum wins), the mean of sn2new there as a fixed-order reduction (k_gs_sum: lane in row order, wave
// butterfly, waves in order; k_vp_reduce over the workgroups in index order), VarThresh = max(1, sn2_avg) (k_gs_thresh).  The start:
// k_gs_start clips W E points -- draws of k_vp_draw or the caller's -- into [LB, UB] (gplite_sample.m:102) and writes them into the
// sampler's walker buffer.  Nothing is atomic, no transcendental is the device library's.
#pragma once
#include "is_sample_kernels.h"   // isp_body, IsPredArgs
#include "vp_tools_kernels.h"

template <int QS>
__global__ void __launch_bounds__(ISP_THREADS) k_gs_pred(IsPredArgs g) {
  isp_body<QS, true>(g, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y);
}

struct GsTargetArgs {
  int S, E, C, nstride;
  const int* ncand;             // candidates of ensemble e at ncand[e * nstride]
  const unsigned char* mask;    // E x C
  const double *ymu, *ys2;      // S x E x C (k_gs_pred)
  const double* vt;             // [0]: VarThresh
  double beta;
  double* val;                  // E x C: what k_is_step consumes
};

// The packed blocks of vbmc_gp_surrogate_sample, from the shape alone (C candidates a round, n0 = W E D, Nnn: 0 without the noise estimate):
//   extra (behind the sampler's E x C values, is_core.h): ymu | ys2, S x E x C each
//   v:  VarThresh | sn2_avg | the sum | the partials of k_gs_sum (VPT_MAXBLK)
//   x0: the start | the same clipped into the box           nn: the draws (Nnn x D) | sn2new at each draw's nearest row
struct GsBlocks {
  DevLayout extra, v, x0, nn;
  DevWin<double> ymu, ys2, vt, sum, part, start, clipped, draws, sn2;
  GsBlocks(int D, int S, int E, int C, size_t n0, int Nnn) {
    ymu = extra.add<double>((size_t)S * E * C); ys2 = extra.add<double>((size_t)S * E * C);
    vt = v.add<double>(2); sum = v.add<double>(1); part = v.add<double>(VPT_MAXBLK);
    start = x0.add<double>(n0); clipped = x0.add<double>(n0);
    draws = nn.add<double>((size_t)Nnn * D); sn2 = nn.add<double>(Nnn);
  }
  void bind(GsTargetArgs& t, IsPredArgs& g, void* dextra, void* dv) const { g.fmu = ymu.at(dextra); g.ys2 = ys2.at(dextra); t.ymu = g.fmu; t.ys2 = g.ys2; t.vt = vt.at(dv); }
};

__global__ void __launch_bounds__(64) k_gs_target(GsTargetArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x, C = a.C, S = a.S;
  const int nc = min(a.ncand[(size_t)e * a.nstride], C);
  if (c >= nc || a.mask[(size_t)e * C + c] == 0) return;
  const size_t o = (size_t)e * C + c, st = (size_t)a.E * C;
  double ybar = a.ymu[o], ys2 = a.ys2[o];
  if (S > 1) {                                       // gplite_pred.m:157, :161-162
    double sy = 0.0, sv = 0.0, vy = 0.0;
    for (int s = 0; s < S; ++s) sy = sy + a.ymu[o + st * s];
    ybar = sy / (double)S;
    for (int s = 0; s < S; ++s) { const double d = a.ymu[o + st * s] - ybar; vy = vy + d * d; }
    vy = vy / (double)(S - 1);
    for (int s = 0; s < S; ++s) sv = sv + a.ys2[o + st * s];
    ys2 = sv / (double)S + vy;
  }
  const double VarThresh = a.vt[0], beta = a.beta;
  double y = ybar;
  if (!((VarThresh == 0.0 || !(fabs(VarThresh) < __builtin_inf())) && beta == 0.0)) {   // gplite_sample.m:111-117
    if (ys2 >= VarThresh) y = ybar - (ys2 - VarThresh);
    y = y - beta * sqrt(ys2);
  }
  if (!(y > -__builtin_inf() && y < __builtin_inf())) y = -__builtin_inf();
  a.val[o] = y;
}

// W E starting points (row r = w + W e of the W E x D column-major buffer) clipped into the box, into the walker buffer and x0_out
__global__ void __launch_bounds__(256) k_gs_start(int W, int D, int E, const double* __restrict__ X0, const double* __restrict__ LB,
                                                  const double* __restrict__ UB, double* __restrict__ x, double* __restrict__ x0c) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = W * E;
  if (i >= n * D) return;
  const int r = i % n, d = i / n, w = r % W, e = r / W;
  const double v = fmin(fmax(X0[i], LB[d]), UB[d]);
  x[((size_t)e * W + w) * D + d] = v;
  x0c[(size_t)w + (size_t)W * (d + (size_t)D * e)] = v;
}

#define GS_SUM_T 256
// partial[b] = the sum of v over the rows b, b + gridDim.x, ... of GS_SUM_T values: lane in row order, wave butterfly, waves in order
__global__ void __launch_bounds__(GS_SUM_T) k_gs_sum(int n, const double* __restrict__ v, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_w[GS_SUM_T / 64];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * GS_SUM_T + tid; i < n; i += (long long)gridDim.x * GS_SUM_T) acc = acc + v[i];
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) s_w[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < GS_SUM_T / 64; ++w) s = s + s_w[w];
    partial[blockIdx.x] = s;
  }
}
// vt[1] = sn2_avg = sum / n (gpsample_vbmc.m:33), vt[0] = VarThresh = max(1, sn2_avg) (:38)
__global__ void k_gs_thresh(const double* __restrict__ sum, int n, double* __restrict__ vt) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double avg = sum[0] / (double)n;
  vt[1] = avg;
  vt[0] = fmax(1.0, avg);
}

struct GsFinishArgs {
  VptPost P;                    // D, and the transform where origflag asks for it (has_tr = 0: the identity)
  int Ns, Nm, E, origflag;
  const double* Xa;             // Nm x D x E
  double* X;                    // Ns x D
};

template <int DT>
__global__ void __launch_bounds__(VPT_T) k_gs_finish(GsFinishArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[DT * VPT_TS];
  __shared__ VptTrS<DT> S;
  const int tid = threadIdx.x, D = a.P.D;
  const long long r = (long long)blockIdx.x * VPT_T + tid;
  for (int j = tid; j < VB_EXP_TAB_N; j += VPT_T) tab[j] = c_exp2_tab[j];
  vpt_stage_tr<DT>(a.P, S, tid);
  __syncthreads();
  if (r >= a.Ns) return;
  const int e = (int)(r % a.E);
  const long long i = r / a.E;
  double* col = stg + tid;
  for (int d = 0; d < D; ++d) col[d * VPT_TS] = a.Xa[(size_t)i + (size_t)a.Nm * (d + (size_t)D * e)];
  double x[DT];
  vpt_finish<DT>(x, a.P, S, a.origflag, col, tab);
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (d < D) a.X[(size_t)r + (size_t)a.Ns * d] = x[d];
}

// The multi-run diagnostics on the device: the pair loop of vbmc_diagnostics.m:116-127 -- vbmc_kldiv.m:72-77 and vbmc_mtv.m on sample
// matrices (infinite mesh bounds, :35-38, :44-47) for every pair of R runs -- with what is per run done once per run.  Run i's draws
// are k_vp_draw's (vp_tools_kernels.h); its mesh, counts, cosine coefficients, bandwidth and inverse transform are mtv_kernels.h's
// kernels over the R D columns, column c = i D + d, and so is the integral of every pair and dimension (k_mtv_integral).  New here:
//   k_diag_cross_kl  the draws of run i against the densities of the runs.  Phase 0 (grid nb x 1): the run's own log density at each
//                    of its points with the rule of vbmc_kldiv.m:75 into own[r].  Phase 1 (grid nb x R): workgroup row j evaluates
//                    posterior j at the same points, applies the rule of :76 and sums log q_j - log q_i: lane in row order, wave
//                    shuffle, waves in order, one partial per workgroup that k_vp_reduce adds in index order.  Row i leaves zeros.
//                    The tile loop, the workgroup count and every operation of a term are k_vp_kldiv's, so entry (i, j) carries
//                    the bits of vbmc_vp_kldiv(vp_i, vp_j, Ns, seed + i) -- except where a density comes within e^40 of the
//                    smallest normal double: there the reference's own value is what rounding left of it, and the kernel forms
//                    the density as the reference does (diag_formed_density).  The own density is evaluated once per point, not R - 1
//                    times; R accumulators per lane would have to be indexed at run time (scratch), so the other posteriors lie
//                    along the grid and each re-reads the D doubles of a point.
//   k_diag_dct       k_mtv_dct's two transforms as the product of the n x n cosine matrix with the n x C block of columns on
//                    v_mfma_f64_16x16x4_f64: A is 16 outputs x 4 inputs of cosines, each folded out of the quarter-wave LDS table ONCE
//                    and used for 32 columns; B is 4 inputs x 16 columns.  A wave owns 16 outputs of 32 columns and walks all n inputs
//                    in index order through one accumulator chain per output, so a column's result depends neither on C nor on the
//                    grid nor on its neighbours (columns beyond C enter as zeros and are not stored).
// Every floating-point sum has a fixed order; nothing depends on the grid, on R or on which other runs are in the call.
#pragma once
#include "mtv_kernels.h"

#define DIAG_MAXR 32              // runs per call

struct DiagKlArgs {
  const VptPost* P;               // R posteriors
  const double* lcmax;            // R: the largest log coefficient of a component, max_k (log w_k - D log sigma_k) + lognf
  int R, i, N, ntile, phase;
  const double* X;                // N x D column-major: run i's draws
  double* own;                    // N: log q_i at the draws after vbmc_kldiv.m:75 (written by phase 0)
  double* partial;                // gridDim.x x R (phase 1)
};

// The transformed-space density as the reference FORMS it (vbmc_pdf.m:56-60): sum_k (nf w_k / sigma_k^D) exp(-d2_k / 2), every
// exponential rounded to the doubles there are -- next to the smallest double that is a handful of bits, below it zero -- before
// its coefficient lifts it.  xs is the scaled transformed-space point vpt_logmix takes.  Every thread of the workgroup calls it.
template <int DT>
__device__ __forceinline__ double diag_formed_density(const double (&xs)[DT], const VptPost& P, double* s_mu, double* s_cst, double* s_is2, const double* tab, int tid) {
#pragma clang fp contract(off)
  constexpr int KC = VPT_CHUNK / DT;
  double y = 0.0;
  for (int k0 = 0; k0 < P.K; k0 += KC) {
    const int kc = min(KC, P.K - k0);
    __syncthreads();
    for (int e = tid; e < kc * DT; e += VPT_T) s_mu[e] = P.mus[(size_t)k0 * DT + e];
    for (int e = tid; e < kc; e += VPT_T) { s_cst[e] = P.cst[k0 + e]; s_is2[e] = P.is2[k0 + e]; }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const double* mk = s_mu + k * DT;
      double q = 0.0;
#pragma unroll
      for (int d = 0; d < DT; ++d) { const double z = xs[d] - mk[d]; q = q + z * z; }
      const double e = vb_exp_tab<0>(fmax(-0.5 * (s_is2[k] * q), -800.0), tab);
      const double c = vb_exp_tab<0>(fmin(fmax(s_cst[k] + P.lognf, -800.0), 800.0), tab);
      y = y + c * e;
    }
  }
  return y;
}

template <int DT>
__global__ void __launch_bounds__(VPT_T) k_diag_cross_kl(DiagKlArgs a) {
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double stg[DT * VPT_TS];
  __shared__ double s_mu[VPT_CHUNK], s_cst[VPT_CHUNK / DT], s_is2[VPT_CHUNK / DT];
  __shared__ double s_w[VPT_T / 64];
  __shared__ VptTrS<DT> S;
  const int tid = threadIdx.x, N = a.N, j = a.phase ? (int)blockIdx.y : a.i;
  if (a.phase && j == a.i) {
    if (tid == 0) a.partial[(size_t)blockIdx.x * a.R + j] = 0.0;
    return;
  }
  const VptPost P = a.P[j];
  const double lcmax = a.lcmax[j];
  const int D = P.D;
  for (int e = tid; e < VB_EXP_TAB_N; e += VPT_T) tab[e] = c_exp2_tab[e];
  vpt_stage_tr<DT>(P, S, tid);
  __syncthreads();
  double acc = 0.0;
  for (int t = blockIdx.x; t < a.ntile; t += gridDim.x) {
    const long long r = (long long)t * VPT_T + tid;
    double u[DT], gn[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) u[d] = (d < D && r < N) ? a.X[(size_t)r + (size_t)N * d] : 0.0;
    // vpt_eval's steps for the original space (origflag = 1, transflag = 0), the mixture and the Jacobian kept apart
    double lj = 0.0;
    if (P.has_tr) {
      vpt_direct<DT>(u, S);
      lj = vpt_logjac<DT>(u, S, tab) + P.ljc;
      if (P.has_rot) vpt_rot<DT>(u, S.R, false, P.D, stg + tid);
      if (P.has_sc) {
#pragma unroll
        for (int d = 0; d < DT; ++d) u[d] = u[d] / S.row[5][d];
      }
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) u[d] = u[d] * P.ilam[d];
    double lt = vpt_logmix<DT, false>(u, P, s_mu, s_cst, s_is2, tab, tid, gn);
    // Where an exponential of the mixture, the mixture itself or the density comes within e^40 of the smallest normal double, the
    // reference's value is what rounding to a few bits (or to zero) left of it, and its logarithm moves with every one of them:
    // there the density is formed as the reference forms it.  (The log-sum-exp form, which k_vp_kldiv keeps throughout, holds
    // full precision there, which the reference does not have.)  The workgroup decides together: the chunks are staged together.
    const bool near = r < N && lt == lt && lj == lj && (!(lt - lcmax >= -660.0) || !(lt >= -668.0) || !(lt - lj >= -668.0));
    double formed = 0.0;
    if (__syncthreads_or(near ? 1 : 0)) formed = diag_formed_density<DT>(u, P, s_mu, s_cst, s_is2, tab, tid);
    if (lt < VPT_LOG_DENORM_MIN) lt = -__builtin_inf();
    const double lq = lt - lj;
    if (r < N) {
#pragma clang fp contract(off)
      // the reference forms the density, replaces a zero or non-finite one, and takes the logarithm (vbmc_kldiv.m:73-77)
      const double q = near ? formed / vb_exp_tab<0>(fmin(fmax(lj, -800.0), 800.0), tab) : vb_exp_tab<0>(fmin(lq, 800.0), tab);
      const bool bad = !(q > 0.0) || !(q < __builtin_inf());
      if (!a.phase) a.own[r] = bad ? 0.0 : vpt_log(q);
      else acc = acc + ((bad ? VPT_LOG_REALMIN : vpt_log(q)) - a.own[r]);
    }
  }
  if (!a.phase) return;                                     // (the whole workgroup: the phase is the launch's)
  acc = vpt_block_sum<VPT_T>(acc, s_w, tid);
  if (tid == 0) a.partial[(size_t)blockIdx.x * a.R + j] = acc;
}

#define DIAG_DCT_T 256            // threads per workgroup: four waves, 64 outputs
#define DIAG_DCT_TC 2             // column tiles of 16 per wave
#define DIAG_DCT_U 8              // steps of four inputs fetched ahead (n is a multiple of 32)

typedef double diag_f64x4 __attribute__((ext_vector_type(4)));

// out_o = f_o sum_i in_i cos(pi m / (2 n)), m = o (2 i + 1) (forward, f_0 = 1, f_o = 2) or i (2 o + 1) (inverse, f = 1), as k_mtv_dct.
// Lane l of a wave holds A[row l & 15][input l >> 4] and B[input l >> 4][column l & 15]; the result sits as
// D[row (l >> 4) + 4 r][column l & 15] in register r.  Grid (n / 64, ceil(C / 32)); dynamic LDS (n + 1) doubles.
__global__ void __launch_bounds__(DIAG_DCT_T) k_diag_dct(MtvDctArgs a, int C) {
  extern __shared__ double s_tab[];
  const int tid = threadIdx.x, n = a.n, lane = tid & 63;
  for (int j = tid; j <= n; j += DIAG_DCT_T) s_tab[j] = a.tab[j];
  __syncthreads();
  const unsigned li = lane & 15, lg = lane >> 4, o0 = (blockIdx.x * (DIAG_DCT_T / 64) + (tid >> 6)) * 16, o = o0 + li;
  const unsigned n2 = 2u * (unsigned)n, m4 = 4u * (unsigned)n - 1u;
  // m of this lane's cosine at input i = lg; four inputs on, m grows by 8 o (forward) resp. 4 (2 o + 1) (inverse).  Modulo 4 n
  // the unsigned wrap-around is harmless.
  unsigned m = a.inverse ? lg * (2u * o + 1u) : o * (2u * lg + 1u);
  const unsigned dm = a.inverse ? 4u * (2u * o + 1u) : 8u * o;
  const double* in[DIAG_DCT_TC];
  bool on[DIAG_DCT_TC];
  diag_f64x4 acc[DIAG_DCT_TC];
#pragma unroll
  for (int t = 0; t < DIAG_DCT_TC; ++t) {
    const int col = (int)blockIdx.y * 16 * DIAG_DCT_TC + 16 * t + (int)li;
    on[t] = col < C;
    in[t] = a.in + (size_t)(on[t] ? col : 0) * n + lg;
    acc[t] = diag_f64x4{0.0, 0.0, 0.0, 0.0};
  }
  // DIAG_DCT_U steps of four inputs at a time: their cosines and their inputs are fetched before the first product needs them
  // (one step's table read and loads would otherwise stand in front of every MFMA); the products follow in input order.
  for (int i0 = 0; i0 < n; i0 += 4 * DIAG_DCT_U) {
    double cv[DIAG_DCT_U], b[DIAG_DCT_U][DIAG_DCT_TC];
#pragma unroll
    for (int u = 0; u < DIAG_DCT_U; ++u) {
      unsigned r = m & m4;
      if (r > n2) r = 2u * n2 - r;                             // cos(2 pi - t) = cos t
      const bool neg = r > (unsigned)n;                        // cos(pi - t) = -cos t
      if (neg) r = n2 - r;
      const double c = s_tab[r];
      cv[u] = neg ? -c : c;
      m += dm;
#pragma unroll
      for (int t = 0; t < DIAG_DCT_TC; ++t) {
        const double v = in[t][i0 + 4 * u];
        b[u][t] = on[t] ? v : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < DIAG_DCT_U; ++u) {
#pragma unroll
      for (int t = 0; t < DIAG_DCT_TC; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv[u], b[u][t], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < DIAG_DCT_TC; ++t) {
    if (!on[t]) continue;
    const size_t base = (size_t)((int)blockIdx.y * 16 * DIAG_DCT_TC + 16 * t + (int)li) * n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned row = o0 + lg + 4u * (unsigned)r;
      double s = acc[t][r];
      if (!a.inverse && row > 0) s = 2.0 * s;
      a.out[base + row] = s;
      if (a.a2) { const double h = 0.5 * s; a.a2[base + row] = h * h; }
    }
  }
}

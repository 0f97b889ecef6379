// gplite GP surrogate on gfx950: the marginal likelihood gplite_nlZ and its gradient, behind the factorisation of gp_factor_kernels.h.
#pragma once
#include "common.h"
#include "device_math.h"

// ------------------------------------------------------------------------------------------
// gplite_nlZ (gplite/private/gplite_core.m:128-275, covfun 1, no integrated mean / output warping)
// ------------------------------------------------------------------------------------------
// Partial sums of the Q-contractions over one 64 x 64 tile of (k, j):
//   Q = Kinv/sl - alpha*alpha'                                  (:240, Kinv = L\(L'\eye(N)))
//   part[d]  = sum Q .* K .* sq_dist(X(:,d)'/ell_d), d < D       (:244-247; the 1/2 is applied in k_nlz_final)
//   part[D]  = sum Q .* K                                       (:248)
//   part[D+1+i] = sum_j dsn2(j,i) Q_jj                          (:257-262)
// K is rebuilt exactly as k_gp_build forms it.  Fixed-order block reduction, no atomics.
#define NLZ_T 64
// One workgroup per 64 x 64 tile (k along the lanes, 16 rows j per wave) of the upper triangle of tiles; off-diagonal
// tiles count twice (Q, K and the distance matrices are symmetric), tiles below the diagonal write zeros.
template <int DT>
__global__ void __launch_bounds__(256) k_nlz_grad(int N, int D, int Nhyp, int Nnoise, const double* __restrict__ hyp,
                                                  const double* __restrict__ Xc, const double* __restrict__ aa,
                                                  const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                                  const double* __restrict__ scal, const double* __restrict__ dsn2,  // B x Nnoise x N
                                                  double* __restrict__ part) {
  __shared__ double red[256];
  __shared__ double TAB[VB_EXP_TAB_N];
  __shared__ double XK[DT * NLZ_T], XJ[DT * NLZ_T];  // [d][point]
  __shared__ double AJ[NLZ_T], ALJ[NLZ_T];
  const int b = blockIdx.z, tid = threadIdx.x, tk = tid & 63, tj = tid >> 6;
  const int k0 = blockIdx.x * NLZ_T, j0 = blockIdx.y * NLZ_T;
  const int P = D + 1 + Nnoise;
  double* o = part + ((size_t)b * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * P;
  if (k0 > j0) {
    for (int p = tid; p < P; p += 256) o[p] = 0.0;
    return;
  }
  const double* h = hyp + (size_t)b * Nhyp;
  const double sf2 = exp(2.0 * h[D]);
  const double isl = 1.0 / scal[b * 4 + 3];
  const double* xs = Xc + (size_t)b * N * D;
  const double* as = aa + (size_t)b * N;
  const double* Kb = Kinv + (size_t)b * N * N;
  const double* al = alpha + (size_t)b * N;
  TAB[tid] = c_exp2_tab[tid];
  for (int e = tid; e < NLZ_T * (DT - D); e += 256) { XK[D * NLZ_T + e] = 0.0; XJ[D * NLZ_T + e] = 0.0; }
  for (int e = tid; e < NLZ_T * D; e += 256) {
    const int pnt = e / D, d = e - pnt * D;
    XK[d * NLZ_T + pnt] = (k0 + pnt < N) ? xs[(size_t)k0 * D + e] : 0.0;
    XJ[d * NLZ_T + pnt] = (j0 + pnt < N) ? xs[(size_t)j0 * D + e] : 0.0;
  }
  if (tid < NLZ_T) {
    AJ[tid] = (j0 + tid < N) ? as[j0 + tid] : 0.0;
    ALJ[tid] = (j0 + tid < N) ? al[j0 + tid] : 0.0;
  }
  __syncthreads();
  double acc[DT], accK = 0.0, accN[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < DT; ++p) acc[p] = 0.0;
  const int k = k0 + tk;
  if (k < N) {
    double xk[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) xk[d] = XK[d * NLZ_T + tk];
    const double ak = as[k], alk = al[k];
    const double sym = (k0 < j0) ? 2.0 : 1.0;
    for (int t = 0; t < 16; ++t) {
      const int jl = tj * 16 + t, j = j0 + jl;
      if (j >= N) break;
      double dot = 0.0;
#pragma unroll
      for (int d = 0; d < DT; ++d) dot = fma(xk[d], XJ[d * NLZ_T + jl], dot);
      const double c = fmax(AJ[jl] + (ak - 2.0 * dot), 0.0);
      const double kv = sf2 * vb_exp_tab<0>(-0.5 * c, TAB);
      const double q = Kb[(size_t)j * N + k] * isl - ALJ[jl] * alk;    // column j read along k (coalesced)
      const double qk = sym * (q * kv);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const double df = XJ[d * NLZ_T + jl] - xk[d];
        acc[d] = fma(qk, df * df, acc[d]);
      }
      accK += qk;
      if (k == j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < Nnoise) accN[i] = dsn2[((size_t)b * Nnoise + i) * N + j] * q;
      }
    }
  }
  // fixed order: VALU butterfly inside a wave, then the four waves in turn -- one barrier for all D + 1 + Nnoise sums
  // (round 4: a block_sum -- twelve ds_bpermute and two barriers -- per sum)
  __shared__ double wr[4][DT + 5];
  {
    const int wv = tid >> 6, ln = tid & 63;
    double v;
#pragma unroll
    for (int d = 0; d < DT; ++d) { v = wave_sum_valu(acc[d]); if (ln == 0) wr[wv][d] = v; }
    v = wave_sum_valu(accK); if (ln == 0) wr[wv][DT] = v;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v = wave_sum_valu(accN[i]); if (ln == 0) wr[wv][DT + 1 + i] = v; }
  }
  __syncthreads();
  if (tid < DT + 5) {
    const double t = ((wr[0][tid] + wr[1][tid]) + wr[2][tid]) + wr[3][tid];
    if (tid < D) o[tid] = t;
    else if (tid == DT) o[D] = t;
    else if (tid > DT && tid - DT - 1 < Nnoise) o[D + 1 + (tid - DT - 1)] = t;
  }
  (void)red;
}

// The closing kernel of gplite_nlZ, one block per hyper-parameter vector:
//   nlZ  = (y-m)'*alpha/2 + sum(log(diag(L))) + N*log(2*pi*sl)/2                                   (gplite_core.m:205)
//   dnlZ = the tile partials of k_nlz_grad summed in tile order (grad != 0), and the mean-function block -dm'*alpha
//          (:274, gplite_meanfun.m:402,406,433-435)
// out = [nlZ B | failure index of the factorisation B | dnlZ B x Nhyp]: the one block that travels back to the host.
// (Round 5: the value, the tile sums and the 2 D + 1 mean-function dot products were two kernels, the second walking them one
// wave per hyper-parameter with dependent loads -- 7 + 15..24 us; now one pass over n per thread, every load of a thread in
// flight at once, wave sums and a fixed-order sum over the four waves.)
template <int DT>
__global__ void __launch_bounds__(256) k_nlz_final(int N, int D, int Nhyp, int Nnoise, int Nmean, int meanfun, int ntile, int grad,
                                                   const double* __restrict__ X, const double* __restrict__ y,
                                                   const double* __restrict__ hyp, const double* __restrict__ A,
                                                   const double* __restrict__ alpha, const double* __restrict__ scal,
                                                   const double* __restrict__ part, const double* __restrict__ pfd,
                                                   double* __restrict__ out) {
  __shared__ double wred[4][2 * DT + 3];
  __shared__ double sxm[DT], som[DT];
  const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = D + 1 + Nnoise, moff = D + 1 + Nnoise;
  const double* hm = hyp + (size_t)b * Nhyp + moff;
  const double* al = alpha + (size_t)b * N;
  const double* Ab = A + (size_t)b * N * N;
  double* g = out + 2 * (size_t)B + (size_t)b * Nhyp;
  if (tid < DT) {
    const bool on = meanfun == 4 && tid < D;
    sxm[tid] = on ? hm[1 + tid] : 0.0;
    som[tid] = on ? exp(hm[D + 1 + tid]) : 1.0;
  }
  if (pfd && tid == 0) out[B + b] = pfd[b];
  __shared__ double tq[4][64];
  if (grad && lane < P) {
    // the tile partials: wave q takes the q-th quarter of the tiles (in tile order, eight loads in flight), the quarters are
    // added in order below
    const int per = (ntile + 3) >> 2, j0 = wave * per, j1 = min(ntile, j0 + per);
    double t = 0.0;
    for (int jt = j0; jt < j1; jt += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = jt + u < j1 ? part[((size_t)b * ntile + jt + u) * P + lane] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) t += v[u];
    }
    tq[wave][lane] = t;
  }
  __syncthreads();
  if (grad && tid < P) {
    const double t = ((tq[0][tid] + tq[1][tid]) + tq[2][tid]) + tq[3][tid];
    const double mult = scal[b * 4 + 1];
    if (tid < D) g[tid] = t / 2.0;                 // sum(sum(Q.*K_temp))/2
    else if (tid == D) g[D] = t;                   // sum(sum(Q.*(2*K_mat)))/2
    else g[tid] = 0.5 * mult * t;                  // 0.5*sn2_mult*sum(dsn2(:,i).*dgQ)
  }
  double t1[DT], t2[DT], t0 = 0.0, quad = 0.0, ld = 0.0;
#pragma unroll
  for (int d = 0; d < DT; ++d) { t1[d] = 0.0; t2[d] = 0.0; }
  for (int n = tid; n < N; n += 256) {
    const double a = al[n], yn = y[n], dg = Ab[(size_t)n * N + n];
    double x[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) x[d] = (meanfun == 4 && d < D) ? X[n + (size_t)N * d] : 0.0;
    double z2 = 0.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const double z = (x[d] - sxm[d]) / som[d];
      z2 = fma(z, z, z2);
      t1[d] = fma(z / som[d], a, t1[d]);           // gplite_meanfun.m:433-435
      t2[d] = fma(z * z, a, t2[d]);
    }
    const double m = meanfun == 0 ? 0.0 : (meanfun == 1 ? hm[0] : hm[0] - 0.5 * z2);    // gplite_meanfun.m:425-431
    quad = fma(yn - m, a, quad);
    ld += log(dg);
    t0 += a;
  }
  // fixed order: butterfly inside a wave, then the four waves in turn
  {
    double v;
    v = wave_sum_valu(t0); if (lane == 0) wred[wave][0] = v;
    v = wave_sum_valu(quad); if (lane == 0) wred[wave][1] = v;
    v = wave_sum_valu(ld); if (lane == 0) wred[wave][2] = v;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      v = wave_sum_valu(t1[d]); if (lane == 0) wred[wave][3 + d] = v;
      v = wave_sum_valu(t2[d]); if (lane == 0) wred[wave][3 + DT + d] = v;
    }
  }
  __syncthreads();
  if (tid < 2 * DT + 3) {
    const double t = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    wred[0][tid] = t;
  }
  __syncthreads();
  if (tid == 0) out[b] = wred[0][1] / 2.0 + wred[0][2] + N * log(2.0 * 3.14159265358979323846 * scal[b * 4 + 3]) / 2.0;
  if (grad && tid < Nmean) {
    const int i = tid;
    double t;
    if (i == 0) t = wred[0][0];
    else if (i <= D) t = wred[0][3 + (i - 1)];
    else t = wred[0][3 + DT + (i - 1 - D)];
    g[moff + i] = -t;
  }
}

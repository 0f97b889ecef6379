// gplite GP surrogate on gfx950, the factorisation: SE-ARD kernel matrix (sq_dist), jittered Cholesky posterior, alpha, rank-one append.
//
// Reference: utils/sq_dist.m:14-50, gplite/private/gplite_core.m:33-102, gplite/gplite_post.m:167-251,
// gplite/gplite_meanfun.m:400-436.
//
//   k_sq_dist_mfma  C = max(|a|^2 + |b|^2 - 2 a'b, 0), the a'b contraction on v_mfma_f64_16x16x4_f64
//   k_gp_build      A_s = K/(sn2div*mult) + diag(sn2/sn2div)   (Lchol)   or  K + mult*diag(sn2)
//   k_chol2         (chol_mfma.h) in-place blocked (16) right-looking Cholesky, upper factor, one WG per sample,
//                   reports MATLAB's p (> 0 = not positive definite) for the jitter retry
//   k_gp_scale      scaled, centred inputs and row norms per hyper-sample; r = y - m(X)
//   k_alpha_solve*  alpha = R \ (R' \ z), one right-hand side per matrix; k_tri_inverse2_alpha: with inv(R')' in the same launch
//   k_rank1_*       the rank-one append of one observation (gplite_post.m:189-245)
#pragma once
#include "chol_mfma.h"
#include "common.h"
#include "device_math.h"
#include "elbo_kernels.h"   // block_sum
#include "trsm_mfma.h"      // TRI2_W, tri_inverse2_body

// ------------------------------------------------------------------------------------------
// sq_dist on MFMA.  a: D x n, b: D x m (column-major, already mean-centred by the caller kernel
// through `mu`), C: n x m.  One wave computes a 16(i) x 16(j) tile as the TRANSPOSED product
// (rows = j from b, cols = i from a) so that the four accumulator registers of a lane are four
// consecutive-j rows of ONE column i... stores of a fixed register are 16 consecutive i (128 B).
// A operand: lane l holds b[d = 4q + (l>>4)][j0 + (l&15)];  B operand: a[d = 4q + (l>>4)][i0 + (l&15)].
// C/D layout of v_mfma_f64_16x16x4_f64: col = l&15, row = (l>>4) + 4*reg.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sq_dist_mfma(int D, int n, int m, const double* __restrict__ a,
                                                      const double* __restrict__ b, const double* __restrict__ mu,
                                                      double* __restrict__ C) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ti = blockIdx.x * 4 + wv;     // tile along i (a)
  const int tj = blockIdx.y;              // tile along j (b)
  const int i0 = ti * 16, j0 = tj * 16;
  if (i0 >= n) return;
  const int li = lane & 15, lq = lane >> 4;
  const int ia = i0 + li, jb = j0 + li;
  vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
  double aa = 0.0, bb = 0.0;  // partial |a_i|^2 (for i = ia) and |b_j|^2 (j = jb) over this lane's d's
  for (int q = 0; q < (D + 3) / 4; ++q) {
    const int d = 4 * q + lq;
    double av = 0.0, bv = 0.0;
    if (d < D) {
      if (ia < n) av = a[d + (size_t)D * ia] - mu[d];
      if (jb < m) bv = b[d + (size_t)D * jb] - mu[d];
    }
    aa = fma(av, av, aa);
    bb = fma(bv, bv, bb);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, av, acc, 0, 0, 0);
  }
  // complete the squared norms across the 4 lanes sharing (l&15)
  aa += __shfl_xor(aa, 16, 64); aa += __shfl_xor(aa, 32, 64);
  bb += __shfl_xor(bb, 16, 64); bb += __shfl_xor(bb, 32, 64);
  // lane holds column i = ia, rows j = j0 + lq + 4*reg ; needs bb of those j (held by lanes with l&15 == lq+4reg)
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int jr = lq + 4 * reg;
    const double bbj = __shfl(bb, jr, 64);
    const int j = j0 + jr;
    if (ia < n && j < m) {
      double c = aa + (bbj - 2.0 * acc[reg]);   // sq_dist.m:45  sum(a.*a)' + (sum(b.*b) - 2*a'*b)
      C[ia + (size_t)n * j] = fmax(c, 0.0);     // :49
    }
  }
}

// ------------------------------------------------------------------------------------------
// device mean function (ids 0, 1, 4) at a point x (strided access), hyp_mean points at the block
// ------------------------------------------------------------------------------------------
__device__ inline double gp_meanfun(int meanfun, int D, const double* hm, const double* x, size_t stride) {
  if (meanfun == 0) return 0.0;
  if (meanfun == 1) return hm[0];
  double z2 = 0.0;
  for (int d = 0; d < D; ++d) {
    double t = (x[d * stride] - hm[1 + d]) / exp(hm[D + 1 + d]);
    z2 = fma(t, t, z2);
  }
  return hm[0] - 0.5 * z2;  // gplite_meanfun.m:425-431
}

// A_s for the Cholesky.  Xc[s] holds the scaled, mean-centred inputs a = (X' ./ ell) - mean  (D x N),
// aa[s][n] = |a_n|^2.  K = sf2 * exp(-max(aa_i + aa_j - 2 a_i.a_j, 0)/2)   (gplite_core.m:52-56)
// rout != null: the residual r = y - m(X) of the same hyper-sample as well (gplite_core.m:58-65; round 4 had a kernel of its own for it).
__global__ void __launch_bounds__(256) k_gp_scale(int N, int D, int Nhyp, const double* __restrict__ X,
                                                  const double* __restrict__ hyp, double* __restrict__ Xc,
                                                  double* __restrict__ aa, int moff, int meanfun, const double* __restrict__ y,
                                                  double* __restrict__ rout) {
  const int s = blockIdx.y;
  const double* h = hyp + (size_t)s * Nhyp;
  __shared__ double mean[32], sell[32], som[32];
  const int tid = threadIdx.x;
  if (rout && meanfun == 4 && tid < D) som[tid] = exp(h[moff + D + 1 + tid]);
  {
    // mean over n of X(n,d)/ell_d  (mean(a,2), sq_dist.m:36): one wave per dimension at a time, lanes along n with the loads
    // of eight rows in flight, fixed-order butterfly.  (Round 5: the first version walked N / 8 dependent load + divide steps
    // per lane and called exp(h[d]) for every element of the scaled copy -- 18 us of a 0.55 ms gplite_nlZ call.)
    const int wave = tid >> 6, lane = tid & 63;
    // wave w takes the dimensions w, w + 4, ...: all of them at once, eight rows per lane and dimension in flight (the ragged end
    // masked: adds + 0), so that the whole reduction is one round trip to memory -- the inputs have just been uploaded
    double ell[8], acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int d = wave + 4 * j; ell[j] = d < D ? exp(h[d]) : 1.0; acc[j] = 0.0; }
    for (int n = lane; n < N; n += 8 * 64) {
      double v[8][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = wave + 4 * j;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[j][u] = (d < D && n + 64 * u < N) ? X[(size_t)N * d + n + 64 * u] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[j] += v[j][u] / ell[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = wave + 4 * j;
      if (d < D) {                       // wave-uniform
        const double t = wave_sum(acc[j]);
        if (lane == 0) { mean[d] = t / N; sell[d] = ell[j]; }
      }
    }
  }
  __syncthreads();
  for (int n = blockIdx.x * blockDim.x + tid; n < N; n += gridDim.x * blockDim.x) {
    double acc = 0.0;
    double xv[32];                                        // the point's coordinates: every load in flight at once
#pragma unroll
    for (int d = 0; d < 32; ++d) xv[d] = d < D ? X[n + (size_t)N * d] : 0.0;
#pragma unroll
    for (int d = 0; d < 32; ++d)
      if (d < D) {
        double v = xv[d] / sell[d] - mean[d];
        Xc[((size_t)s * N + n) * D + d] = v;
        acc = fma(v, v, acc);
      }
    aa[(size_t)s * N + n] = acc;
    if (rout) {
      const double* hm = h + moff;
      double m = 0.0;
      if (meanfun == 1) m = hm[0];
      else if (meanfun == 4) {
        double z2 = 0.0;
#pragma unroll
        for (int d = 0; d < 32; ++d)
          if (d < D) {
            const double t = (xv[d] - hm[1 + d]) / som[d];
            z2 = fma(t, t, z2);
          }
        m = hm[0] - 0.5 * z2;            // gplite_meanfun.m:425-431
      }
      rout[(size_t)s * N + n] = y[n] - m;
    }
  }
}

// One workgroup per 64 x 64 tile of the UPPER triangle (k_chol2 reads i <= j only; it zeroes the strict lower part
// itself): both 64-point slabs of the scaled inputs are staged in LDS dimension-major, a lane keeps its own point in
// registers and walks 16 columns whose coordinates are wave-uniform LDS broadcasts; exponent by the table exp.
#define GPB_T 64
template <int DT>   // D padded to DT with zero coordinates: the dimension loops are branch-free
__global__ void __launch_bounds__(256) k_gp_build(int N, int D, int Nhyp, const double* __restrict__ hyp,
                                                  const double* __restrict__ Xc, const double* __restrict__ aa,
                                                  const double* __restrict__ sn2,      // S x N  noise variance per point
                                                  const double* __restrict__ scal,     // S x 4: sn2div, mult, lchol, _
                                                  const unsigned char* __restrict__ active, double* __restrict__ A) {
  const int s = blockIdx.z;
  if (!active[s]) return;
  const int i0 = blockIdx.x * GPB_T, j0 = blockIdx.y * GPB_T;
  if (i0 > j0) return;                               // tile entirely below the diagonal
  __shared__ double TAB[VB_EXP_TAB_N];
  __shared__ double XI[DT * GPB_T], XJ[DT * GPB_T];  // [d][point]
  __shared__ double AJ[GPB_T];
  const int tid = threadIdx.x, ti = tid & 63, tj = tid >> 6;
  const double* h = hyp + (size_t)s * Nhyp;
  const double sf2 = exp(2.0 * h[D]);
  const double sn2div = scal[s * 4 + 0], mult = scal[s * 4 + 1];
  const bool lchol = scal[s * 4 + 2] != 0.0;
  const double* xs = Xc + (size_t)s * N * D;
  const double* as = aa + (size_t)s * N;
  double* As = A + (size_t)s * N * N;
  TAB[tid] = c_exp2_tab[tid];
  // the rows i0 .. i0+63 of the point-major Xc are one contiguous block: coalesced reads, transposed into LDS
  for (int e = tid; e < GPB_T * (DT - D); e += 256) { XI[D * GPB_T + e] = 0.0; XJ[D * GPB_T + e] = 0.0; }   // padded dimensions
  for (int e = tid; e < GPB_T * D; e += 256) {
    const int pnt = e / D, d = e - pnt * D;
    XI[d * GPB_T + pnt] = (i0 + pnt < N) ? xs[(size_t)i0 * D + e] : 0.0;
    XJ[d * GPB_T + pnt] = (j0 + pnt < N) ? xs[(size_t)j0 * D + e] : 0.0;
  }
  if (tid < GPB_T) AJ[tid] = (j0 + tid < N) ? as[j0 + tid] : 0.0;
  __syncthreads();
  const int i = i0 + ti;
  if (i >= N) return;
  double xi[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) xi[d] = XI[d * GPB_T + ti];
  const double ai = as[i];
  const double sdiv = sn2div * mult;
  for (int t = 0; t < 16; ++t) {
    const int jl = tj * 16 + t, j = j0 + jl;
    if (j >= N) break;
    double dot = 0.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) dot = fma(xi[d], XJ[d * GPB_T + jl], dot);
    const double c = fmax(ai + (AJ[jl] - 2.0 * dot), 0.0);
    const double k = sf2 * vb_exp_tab<0>(-0.5 * c, TAB);
    double v;
    if (lchol) v = k / sdiv + (i == j ? sn2[(size_t)s * N + i] / sn2div : 0.0);  // :78
    else v = k + (i == j ? mult * sn2[(size_t)s * N + i] : 0.0);               // :92
    As[(size_t)j * N + i] = v;
  }
}

// D -> padded DT for k_gp_build / k_nlz_grad
#define DISPATCH_GPDT(D_, ...)                                   \
  do {                                                           \
    if ((D_) <= 4) { constexpr int DT = 4; __VA_ARGS__; }        \
    else if ((D_) <= 8) { constexpr int DT = 8; __VA_ARGS__; }   \
    else if ((D_) <= 12) { constexpr int DT = 12; __VA_ARGS__; } \
    else if ((D_) <= 16) { constexpr int DT = 16; __VA_ARGS__; } \
    else if ((D_) <= 24) { constexpr int DT = 24; __VA_ARGS__; } \
    else { constexpr int DT = 32; __VA_ARGS__; }                 \
  } while (0)

// ------------------------------------------------------------------------------------------
// Blocked right-looking Cholesky, upper factor R (R'R = A) in place, strict lower part zeroed: k_chol2 in chol_mfma.h.
// pfail[s] = 0 on success, j+1 when the j-th pivot is not positive (MATLAB's [R,p] = chol(A)).
// ------------------------------------------------------------------------------------------

// alpha-type solve x = R \ (R' \ z) for ONE right-hand side per matrix, latency-shaped: one 1024-thread workgroup per
// matrix, the vector in LDS.  Per 16-row block step the 16 dot products with the already solved part are one wave each
// (lanes along the long dimension, fixed-order butterfly), then wave 0 applies the precomputed inverse of the diagonal
// block (k_diag_inv).  ~2 us per step instead of ~5 us for the 16-column MFMA slab solve with 15 zero columns.
#define ASOLVE_THREADS 1024
// skip_fwd != 0: Zin already holds R' \ z (the factorisation solved it on the way, chol_mfma.h): backward half only.
__global__ void __launch_bounds__(ASOLVE_THREADS) k_alpha_solve(int N, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                                const unsigned char* __restrict__ on, const double* __restrict__ Zin,
                                                                double* __restrict__ Xo, int skip_fwd, const double* __restrict__ scal) {
  extern __shared__ double lds[];   // Np + 16
  const int s = blockIdx.x;
  if (!on[s]) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nblk = (N + 15) >> 4, Np = nblk << 4;
  double* v = lds;
  double* tmp = v + Np;
  const double* R = Lall + (size_t)s * N * N;
  const double* Fi = Finv + (size_t)s * nblk * 256;
  for (int i = tid; i < Np; i += ASOLVE_THREADS) v[i] = i < N ? Zin[(size_t)s * N + i] : 0.0;
  __syncthreads();
  // ---- forward: R' v = z
  for (int bi = skip_fwd ? nblk : 0; bi < nblk; ++bi) {
    const int b0 = bi << 4, c = b0 + wave;
    double dot = 0.0;
    if (c < N)
      for (int row = lane; row < b0; row += 64) dot = fma(R[(size_t)c * N + row], v[row], dot);
    dot = wave_sum(dot);
    if (lane == 0) tmp[wave] = v[c < Np ? c : 0] - dot;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) a = fma(Fi[(size_t)bi * 256 + tid * 16 + cc], tmp[cc], a);
      v[b0 + tid] = (b0 + tid < N) ? a : 0.0;
    }
    __syncthreads();
  }
  // ---- backward: R x = v
  for (int bi = nblk - 1; bi >= 0; --bi) {
    const int b0 = bi << 4, e0 = b0 + 16, i = b0 + wave;
    double dot = 0.0;
    if (i < N)
      for (int j = e0 + lane; j < N; j += 64) dot = fma(R[(size_t)j * N + i], v[j], dot);
    dot = wave_sum(dot);
    if (lane == 0) tmp[wave] = v[i < Np ? i : 0] - dot;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) a = fma(Fi[(size_t)bi * 256 + cc * 16 + tid], tmp[cc], a);   // (R_bb^{-1})[i][c] = Finv[c][i]
      v[b0 + tid] = (b0 + tid < N) ? a : 0.0;
    }
    __syncthreads();
  }
  const double sl = scal ? scal[s * 4 + 3] : 1.0;     // alpha = x / sl (gplite_core.m:102); no divisor, no division
  for (int i = tid; i < N; i += ASOLVE_THREADS) Xo[(size_t)s * N + i] = scal ? v[i] / sl : v[i];
}

// The same solve for N <= ASOLVE1_THREADS, right-looking: thread e owns element e of the vector in a register.  Per 16-row block step the
// 16 owner lanes (one wave) exchange their entries through LDS and apply the inverse of the diagonal block -- no workgroup
// barrier inside that --, publish x_b, and after ONE barrier every thread behind (forward) / ahead of (backward) the block
// subtracts its 16-term product with x_b.  The 16 matrix entries a thread needs for the NEXT step (and the owner lanes' row
// of the block inverse) are fetched before the barrier: no L2 round trip on the critical path, no 64-lane reduction.
// (k_alpha_solve above stays as the path for larger N; 512 threads: the 32 prefetched values need the 256-VGPR budget.)
#define ASOLVE1_THREADS 512
__device__ __forceinline__ void alpha_solve1_body(int N, int s, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                  const double* __restrict__ Zin, double* __restrict__ Xo, int skip_fwd,
                                                  const double* __restrict__ scal) {
  __shared__ double xb[2][16], tb[16];
  const int e = threadIdx.x, lane = e & 63, k = e & 15, myblk = e >> 4;
  const int nblk = (N + 15) >> 4;
  const double* R = Lall + (size_t)s * N * N;
  const double* Fi = Finv + (size_t)s * nblk * 256;
  double z = e < N ? Zin[(size_t)s * N + e] : 0.0;
  double pre[16], fi[16];
  // ---- forward: R' v = z.  Step b needs R[b0 + r][e] (column e, 16 contiguous rows) for e >= b0 + 16.
  auto fetch_fwd = [&](int b) {
    const int b0 = b << 4;
    const bool mine = e >= b0 + 16 && e < N && b < nblk;
    // 16 contiguous rows of column e: 16-byte loads (a lane per column means every load instruction touches 64 cache lines;
    // half as many instructions as with 8-byte loads).  The last block of a ragged N goes element by element.
    typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
    if (b0 + 16 <= N) {
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        d2u v2 = {0.0, 0.0};
        if (mine) v2 = *reinterpret_cast<const d2u*>(R + (size_t)e * N + b0 + r);
        pre[r] = v2[0]; pre[r + 1] = v2[1];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) pre[r] = (mine && b0 + r < N) ? R[(size_t)e * N + b0 + r] : 0.0;
    }
    if (myblk == b + 1 && b + 1 < nblk) {
#pragma unroll
      for (int c = 0; c < 16; ++c) fi[c] = Fi[(size_t)(b + 1) * 256 + k * 16 + c];      // row k of (R_bb')^{-1}
    }
  };
  if (!skip_fwd) {
  if (myblk == 0) {
#pragma unroll
    for (int c = 0; c < 16; ++c) fi[c] = Fi[k * 16 + c];
  }
  fetch_fwd(0);
  }
  for (int b = skip_fwd ? nblk : 0; b < nblk; ++b) {
    if (myblk == b) {                     // 16 lanes of one wave
      tb[k] = z;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      double a4[4] = {0.0, 0.0, 0.0, 0.0};          // four short chains instead of one of 16 dependent FMAs
#pragma unroll
      for (int c = 0; c < 16; ++c) a4[c & 3] = fma(fi[c], tb[c], a4[c & 3]);
      const double a = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      z = e < N ? a : 0.0;
      xb[b & 1][k] = z;
    }
    // LDS-only barrier: __syncthreads() would also wait for the global loads just issued for the next step (vmcnt(0))
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    double p4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 16; ++r) p4[r & 3] = fma(pre[r], xb[b & 1][r], p4[r & 3]);   // zero for the threads at or before the block
    z -= (p4[0] + p4[1]) + (p4[2] + p4[3]);
    fetch_fwd(b + 1);
  }
  __syncthreads();
  // ---- backward: R x = v.  Step b needs R[e][b0 + c] (row e, 16 columns) for e < b0 -- fetched FOUR steps ahead into a ring
  // (round 5: a step is ~0.25 us of exchange and two 16-term products, an L2 round trip ~1 us; with one step of look-ahead every
  // step waited for its row, 1.2 us per step)
  double prq[4][16];
  auto fetch_bwd = [&](int b, double (&pr)[16]) {
    const int b0 = b << 4;
    const bool mine = b >= 0 && e < b0;
#pragma unroll
    for (int c = 0; c < 16; ++c) pr[c] = (mine && b0 + c < N) ? R[(size_t)(b0 + c) * N + e] : 0.0;
    if (b >= 1 && myblk == b - 1) {
#pragma unroll
      for (int c = 0; c < 16; ++c) fi[c] = Fi[(size_t)(b - 1) * 256 + c * 16 + k];      // row k of R_bb^{-1} = column k of (R_bb')^{-1}
    }
  };
  if (myblk == nblk - 1) {
#pragma unroll
    for (int c = 0; c < 16; ++c) fi[c] = Fi[(size_t)(nblk - 1) * 256 + c * 16 + k];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) fetch_bwd(nblk - 1 - q, prq[q]);
  for (int bb = nblk - 1; bb >= 0; bb -= 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = bb - q;
      if (b >= 0) {                          // uniform
        if (myblk == b) {
          tb[k] = z;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          double a4[4] = {0.0, 0.0, 0.0, 0.0};          // four short chains instead of one of 16 dependent FMAs
#pragma unroll
          for (int c = 0; c < 16; ++c) a4[c & 3] = fma(fi[c], tb[c], a4[c & 3]);
          const double a = (a4[0] + a4[1]) + (a4[2] + a4[3]);
          z = e < N ? a : 0.0;
          xb[b & 1][k] = z;
        }
        // LDS-only barrier: __syncthreads() would also wait for the global loads in flight for the next steps (vmcnt(0))
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        double p4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 16; ++c) p4[c & 3] = fma(prq[q][c], xb[b & 1][c], p4[c & 3]);
        z -= (p4[0] + p4[1]) + (p4[2] + p4[3]);
        fetch_bwd(b - 4, prq[q]);
      }
    }
  }
  if (e < N) Xo[(size_t)s * N + e] = scal ? z / scal[s * 4 + 3] : z;
}
__global__ void __launch_bounds__(ASOLVE1_THREADS, 2) k_alpha_solve1(int N, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                                 const unsigned char* __restrict__ on, const double* __restrict__ Zin,
                                                                 double* __restrict__ Xo, int skip_fwd, const double* __restrict__ scal) {
  const int s = blockIdx.x;
  if (!on[s]) return;
  alpha_solve1_body(N, s, Lall, Finv, Zin, Xo, skip_fwd, scal);
}

// T' = inv(R')' for the marginal-likelihood gradient AND alpha's backward solve in ONE launch (N <= ASOLVE1_THREADS, few
// matrices): workgroups 0 .. nblk - 1 of a matrix invert the factor slab by slab (tri_inverse2_body), workgroup nblk runs the
// single-vector solve.  Neither needs the other; as two kernels on two streams they cost an event record, two stream waits
// and their idle gaps (~12 us of a 0.46 ms gplite_nlZ call) on top of the longer of the two.
static_assert(ASOLVE1_THREADS == 64 * TRI2_W, "the combined launch runs both bodies with one block size");
template <int MAXS>
__global__ void __launch_bounds__(64 * TRI2_W, 2) k_tri_inverse2_alpha(int N, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                                    const unsigned char* __restrict__ on, double* __restrict__ TT,
                                                                    const double* __restrict__ Zin, double* __restrict__ Xo,
                                                                    const double* __restrict__ scal) {
  const int s = blockIdx.y;
  if (!on[s]) return;
  if ((int)blockIdx.x == (int)gridDim.x - 1) alpha_solve1_body(N, s, Lall, Finv, Zin, Xo, 1, scal);
  else tri_inverse2_body<MAXS, (MAXS <= 4 ? 4 : 2)>(N, blockIdx.x, s, Lall, Finv, TT, 1);
}

// [mstar, vstar] = gplite_pred(gp, xstar, ystar, [], 1, 1) (gplite_post.m:189) from the solves the append needs anyway:
//   mstar = m(xstar) + Ks' alpha                                                         (gplite_pred.m:83)
//   vstar = max(fs2, 0) + sn2_eff,  fs2 = kss - |v|^2/sn2_eff (factor) or kss + Ks' x (stored inverse)   (:99-104,120-121)
// and the coefficient (mstar - ystar)/vstar of the alpha update; writes them over sc[s][2], sc[s][3].
__global__ void __launch_bounds__(256) k_rank1_stats(int N, int D, int Nhyp, int moff, int meanfun, const double* __restrict__ hyp,
                                                     const double* __restrict__ xstar, const double* __restrict__ alpha,
                                                     const unsigned char* __restrict__ lchol, const double* __restrict__ Ks,
                                                     const double* __restrict__ V, const double* __restrict__ Xs, double ystar,
                                                     double* __restrict__ sc) {
  __shared__ double red[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool ch = lchol[s] != 0;
  const double* ks = Ks + (size_t)s * N;
  double d1 = 0.0, d2 = 0.0;
  for (int n = tid; n < N; n += 256) {
    d1 = fma(ks[n], alpha[(size_t)s * N + n], d1);
    const double t = ch ? V[(size_t)s * N + n] : 0.0;
    d2 = ch ? fma(t, t, d2) : fma(ks[n], Xs[(size_t)s * N + n], d2);
  }
  d1 = block_sum(d1, red);
  d2 = block_sum(d2, red);
  if (tid == 0) {
    const double sn2 = sc[s * 4 + 0], kss = sc[s * 4 + 1];
    const double mstar = gp_meanfun(meanfun, D, hyp + (size_t)s * Nhyp + moff, xstar, 1) + d1;
    const double fs2 = ch ? kss - d2 / sn2 : kss + d2;
    const double vstar = fmax(fs2, 0.0) + sn2;
    sc[s * 4 + 2] = (mstar - ystar) / vstar;
    sc[s * 4 + 3] = vstar;
  }
}

// Rank-one append of one observation (gplite/gplite_post.m:226-245): column j of the new (N+1) x (N+1) matrix per workgroup.
//   factor samples:   Lnew = [L, v/sn2_eff; 0, sqrt(1 + Kss/sn2_eff - |v/sn2_eff|^2)]            (:228-232)
//   inverse samples:  Lnew = [L + vv*au', -vv; -vv', -1/vstar],  au = -x, vv = -au/vstar          (:234-236)
//   alpha_new = [alpha; 0] + (mstar - ystar)/vstar * [au; -1],   au = x/sn2_eff (factor) or -x     (:227,234,245)
// sc[s] = {sn2_eff, Kss, (mstar - ystar)/vstar, vstar}.
__global__ void __launch_bounds__(256) k_rank1_assemble(int N, const double* __restrict__ Lall, const double* __restrict__ alpha,
                                                        const unsigned char* __restrict__ lchol, const double* __restrict__ V,
                                                        const double* __restrict__ Xs, const double* __restrict__ sc,
                                                        double* __restrict__ Lnew, double* __restrict__ anew) {
  __shared__ double red[256];
  const int j = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, N1 = N + 1;
  const double sn2 = sc[s * 4 + 0], Kss = sc[s * 4 + 1], coef = sc[s * 4 + 2], vstar = sc[s * 4 + 3];
  const bool ch = lchol[s] != 0;
  const double* L = Lall + (size_t)s * N * N;
  const double* v = V + (size_t)s * N;
  const double* x = Xs + (size_t)s * N;
  double* o = Lnew + (size_t)s * N1 * N1 + (size_t)j * N1;
  if (j < N) {
    const double xj = x[j];
    for (int i = tid; i < N; i += 256) o[i] = ch ? L[(size_t)j * N + i] : L[(size_t)j * N + i] - x[i] * xj / vstar;
    if (tid == 0) o[N] = ch ? 0.0 : -xj / vstar;
    // alpha, one entry per column block
    if (tid == 1) anew[(size_t)s * N1 + j] = alpha[(size_t)s * N + j] + coef * (ch ? xj / sn2 : -xj);
  } else {
    double part = 0.0;
    for (int i = tid; i < N; i += 256) {
      const double c = ch ? v[i] / sn2 : -x[i] / vstar;
      o[i] = c;
      part = fma(c, c, part);
    }
    const double cc = block_sum(part, red);
    if (tid == 0) {
      o[N] = ch ? sqrt(1.0 + Kss / sn2 - cc) : -1.0 / vstar;
      anew[(size_t)s * N1 + N] = -coef;
    }
  }
}

__global__ void k_negate_copy(size_t n, const double* __restrict__ src, double* __restrict__ dst) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = -src[i];
}

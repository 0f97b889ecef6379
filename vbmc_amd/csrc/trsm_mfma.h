// Wave-level blocked triangular solves with 16 right-hand sides on v_mfma_f64_16x16x4_f64.
//
// R is the upper Cholesky factor of gplite (MATLAB chol convention, R'R = A), N x N column-major in
// global memory; the N x 16 slab of right-hand sides lives in LDS as V[row * TR_VS + col] (rows padded
// to a multiple of 16 with zeros).  Per 16-row block the trailing update
//     rhs_b -= R[0:b0, b]' * V[0:b0, :]      (forward, R' V = Z)
//     rhs_b -= R[b, e0:N] * X[e0:N, :]       (backward, R X = V)
// is a (16 x b0) x (b0 x 16) product accumulated by one MFMA per 4 rows of the inner dimension; the
// 16 x 16 diagonal block is applied as four more MFMAs with its precomputed inverse (k_diag_inv: 16-step
// substitution once per block, not once per block per column tile).  Used by gplite_pred's V = L' \ (sW .* Ks)
// (gplite/gplite_pred.m:99), the BQ variance (misc/gplogjoint.m:277,318), alpha = L \ (L' \ (y-m))
// (gplite/private/gplite_core.m:102) and the rank-1 update (gplite/gplite_post.m:227-229).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "../../include/vbmc_hip.h"   // VBMC_VARSOLVE_* (trsm_form_for)

typedef double tmf4 __attribute__((ext_vector_type(4)));
#define TR_VS 17  // LDS row stride of the 16-column right-hand-side slab and of the panel buffer (16 columns + 1 pad)
// Narrow slabs for large N: the slab of a wave holds CW = 16, 8 or 4 right-hand sides (row stride CW + 1), the MFMAs still
// run 16 columns wide with zeros beyond CW.  16 columns fit the 160 KB of LDS up to N = 1136, 8 up to N = 2144, 4 up to
// N = 3872 (VBMC's default MaxFunEvals = 50 (2 + D) reaches N = 1700 at D = 32), and -- round 5 -- 2 up to N = 6800, 1 up to
// N = 9696: a fallback that trades matrix-core utilisation for range, chosen per call by trsm_cw_for(N).
template <int CW>
__device__ __forceinline__ double trsm_vld(const double* __restrict__ V, int row, int li) {
  return (CW == 16 || li < CW) ? V[row * (CW + 1) + (CW == 16 ? li : (li < CW ? li : 0))] : 0.0;
}
template <int CW>
__device__ __forceinline__ void trsm_vst(double* __restrict__ V, int row, int li, double x) {
  if (CW == 16 || li < CW) V[row * (CW + 1) + li] = x;
}

// k_diag_inv: Finv[s][b] = (R_bb')^{-1} for every 16 x 16 diagonal block of the upper factor (identity rows beyond
// N), row-major 16 x 16.  The blocked solves apply it with four MFMAs instead of a 16-step substitution chain;
// R_bb^{-1} (backward solve) is its transpose.  One wave per block: lane c < 16 solves R_bb' x = e_c.
__global__ void __launch_bounds__(64) k_diag_inv(int N, const double* __restrict__ Lall, const unsigned char* __restrict__ lchol,
                                                 double* __restrict__ Finv) {
  __shared__ double Rd[256];
  const int bi = blockIdx.x, s = blockIdx.y, lane = threadIdx.x, b0 = bi << 4;
  const int nblk = gridDim.x;
  double* out = Finv + ((size_t)s * nblk + bi) * 256;
  if (!lchol[s]) return;
  const double* Rm = Lall + (size_t)s * N * N;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = lane + 64 * t, ii = e >> 4, jj = e & 15;
    double v = (ii == jj) ? 1.0 : 0.0;
    if (b0 + ii < N && b0 + jj < N && ii <= jj) v = Rm[(size_t)(b0 + jj) * N + b0 + ii];
    Rd[e] = v;
  }
  __syncthreads();
  if (lane < 16) {
    double x[16];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) {   // (R')x = e_c : x_ii = (e_c[ii] - sum_{jj<ii} R[jj][ii] x_jj) / R[ii][ii]
      double t = (ii == lane) ? 1.0 : 0.0;
#pragma unroll
      for (int jj = 0; jj < ii; ++jj) t = fma(-Rd[jj * 16 + ii], x[jj], t);
      x[ii] = t / Rd[ii * 17];
    }
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) out[ii * 16 + lane] = x[ii];   // Finv[ii][c]
  }
}

// The slab and the panel buffer of a solve belong to ONE wave: ordering its LDS writes before its later reads needs a
// wave-level fence, not a workgroup barrier -- which lets several waves of a workgroup run solves of different length.
__device__ __forceinline__ void trsm_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// forward substitution R' V = Z for the slab in LDS (in place)
// bi_start > 0: the slab is known to be zero above row 16 * bi_start (columns of the identity), so is the solution:
// the substitution starts there and the trailing updates skip the zero rows.
template <int CW = 16>
__device__ __forceinline__ void trsm_fwd_wave(int N, const double* __restrict__ Rm, const double* __restrict__ Finv,
                                              double* __restrict__ V, double* __restrict__ P, int lane, int bi_start = 0) {
  const int li = lane & 15, lg = lane >> 4;
  const int nblk = (N + 15) >> 4;
  const int r0 = bi_start << 4;
  for (int bi = bi_start; bi < nblk; ++bi) {
    const int b0 = bi << 4;
    // trailing update: the b0 x 16 panel R[0:b0, b0:b0+16] is streamed through LDS in 64-row chunks with
    // fully coalesced loads (lane = row, one load per column, all 16 in flight), then consumed by MFMAs
    tmf4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    double fv[4];   // A[i = li][k = 4u + lg] = Finv_b[li][4u + lg]
#pragma unroll
    for (int u = 0; u < 4; ++u) fv[u] = Finv[(size_t)bi * 256 + li * 16 + 4 * u + lg];
    double pv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) pv[c] = (r0 + lane < b0 && b0 + c < N) ? Rm[(size_t)(b0 + c) * N + r0 + lane] : 0.0;
    for (int j0 = r0; j0 < b0; j0 += 64) {
      const int nrow = min(64, b0 - j0);
      trsm_wsync();
#pragma unroll
      for (int c = 0; c < 16; ++c) P[lane * TR_VS + c] = pv[c];
      trsm_wsync();
      // prefetch the next chunk of the panel while this one feeds the matrix core
      const int jn = j0 + 64;
#pragma unroll
      for (int c = 0; c < 16; ++c) pv[c] = (jn + lane < b0 && b0 + c < N) ? Rm[(size_t)(b0 + c) * N + jn + lane] : 0.0;
      // nrow is a multiple of 16: four MFMAs per step, their eight LDS operands fetched before the first issues
      for (int jj = 0; jj < nrow; jj += 16) {
        double pa[4], pb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          pa[u] = P[(jj + 4 * u + lg) * TR_VS + li];
          pb[u] = trsm_vld<CW>(V, j0 + jj + 4 * u + lg, li);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[0], pb[0], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[1], pb[1], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[2], pb[2], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[3], pb[3], acc2, 0, 0, 0);
      }
    }
    acc += acc2;
    // v_b = (R_bb')^{-1} (z_b - update): rhs through LDS into the B-operand layout, four MFMAs with Finv
#pragma unroll
    for (int r = 0; r < 4; ++r) trsm_vst<CW>(V, b0 + lg + 4 * r, li, trsm_vld<CW>(V, b0 + lg + 4 * r, li) - acc[r]);
    trsm_wsync();
    tmf4 vb = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u)
      vb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[u], trsm_vld<CW>(V, b0 + 4 * u + lg, li), vb, 0, 0, 0);
    trsm_wsync();
#pragma unroll
    for (int r = 0; r < 4; ++r) trsm_vst<CW>(V, b0 + lg + 4 * r, li, vb[r]);
    trsm_wsync();
  }
}

// backward substitution R X = V for the slab in LDS (in place)
// bi_stop > 0: only the rows from 16 * bi_stop down are wanted (the lower triangle of a symmetric solution)
template <int CW = 16>
__device__ __forceinline__ void trsm_bwd_wave(int N, const double* __restrict__ Rm, const double* __restrict__ Finv,
                                              double* __restrict__ V, int lane, int bi_stop = 0) {
  const int li = lane & 15, lg = lane >> 4;
  const int nblk = (N + 15) >> 4;
  const int Np = nblk << 4;
  for (int bi = nblk - 1; bi >= bi_stop; --bi) {
    const int b0 = bi << 4;
    // trailing update: A[i = li][k = lg] = R[b0+li][j] -- 16 consecutive doubles per inner index (coalesced);
    // eight independent loads are issued per batch to cover the L2 latency
    tmf4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    const bool rv = b0 + li < N;
    double fv[4];   // A[i = li][k = 4u + lg] = (R_bb^{-1})[li][4u + lg] = Finv_b[4u + lg][li]
#pragma unroll
    for (int u = 0; u < 4; ++u) fv[u] = Finv[(size_t)bi * 256 + (4 * u + lg) * 16 + li];
    for (int j0 = b0 + 16; j0 < Np; j0 += 32) {
      double av[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 4 * u + lg;
        av[u] = (rv && j < N) ? Rm[(size_t)j * N + b0 + li] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        if (j0 + 4 * u < Np) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], trsm_vld<CW>(V, j0 + 4 * u + lg, li), acc, 0, 0, 0);
        if (j0 + 4 * (u + 1) < Np) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1], trsm_vld<CW>(V, j0 + 4 * (u + 1) + lg, li), acc2, 0, 0, 0);
      }
    }
    acc += acc2;
    // x_b = R_bb^{-1} (v_b - update) = Finv_b' * rhs
#pragma unroll
    for (int r = 0; r < 4; ++r) trsm_vst<CW>(V, b0 + lg + 4 * r, li, trsm_vld<CW>(V, b0 + lg + 4 * r, li) - acc[r]);
    trsm_wsync();
    tmf4 xb = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u)
      xb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[u], trsm_vld<CW>(V, b0 + 4 * u + lg, li), xb, 0, 0, 0);
    trsm_wsync();
#pragma unroll
    for (int r = 0; r < 4; ++r) trsm_vst<CW>(V, b0 + lg + 4 * r, li, xb[r]);
    trsm_wsync();
  }
}

// ------------------------------------------------------------------------------------------
// Standalone kernels: Z is laid out [r][s][k][N] (column k of the right-hand sides contiguous);
// one wave per (16 columns, hyper-sample s, restart r).  lchol[s] == 0 samples are skipped.
// ------------------------------------------------------------------------------------------
template <int CW = 16>
__device__ __forceinline__ void trsm_slab_load(int N, int K, int k0, const double* __restrict__ Zs, double* __restrict__ V, int lane) {
  const int Np = ((N + 15) >> 4) << 4;
  for (int c = 0; c < CW; ++c) {
    const bool cv = k0 + c < K;
    for (int i = lane; i < Np; i += 64) V[i * (CW + 1) + c] = (cv && i < N) ? Zs[(size_t)(k0 + c) * N + i] : 0.0;
  }
  __syncthreads();
}
template <int CW = 16>
__device__ __forceinline__ void trsm_slab_store(int N, int K, int k0, double* __restrict__ Zs, const double* __restrict__ V, int lane) {
  for (int c = 0; c < CW; ++c) {
    if (k0 + c >= K) break;
    for (int i = lane; i < N; i += 64) Zs[(size_t)(k0 + c) * N + i] = V[i * (CW + 1) + c];
  }
}
#define TRSM_LDS_BYTES_CW(N, CW) ((size_t)(((((N) + 15) >> 4) << 4) * ((CW) + 1) + 64 * TR_VS) * sizeof(double))
#define TRSM_LDS_BYTES(N) TRSM_LDS_BYTES_CW(N, 16)
#define TRSM_NBLK(N) (((N) + 15) >> 4)
// slab width for a problem of N rows: the widest that fits the 160 KB of LDS (0: none does)
static inline int trsm_cw_for(int N) {
  if (TRSM_LDS_BYTES_CW(N, 16) <= 160 * 1024) return 16;
  if (TRSM_LDS_BYTES_CW(N, 8) <= 160 * 1024) return 8;
  if (TRSM_LDS_BYTES_CW(N, 4) <= 160 * 1024) return 4;
  if (TRSM_LDS_BYTES_CW(N, 2) <= 160 * 1024) return 2;      // (round 5) up to N = 6800
  if (TRSM_LDS_BYTES_CW(N, 1) <= 160 * 1024) return 1;      //           up to N = 9696: one right-hand side per wave
  return 0;
}
// the largest N the solves take (whole 16-row blocks): 9696 -- what vbmc_get_limits reports and the refusals quote.  (Rounds 5's texts
// said 10208, which forgot the 64 x TR_VS panel buffer beside the one-column slab.)
static inline int trsm_max_n() {
  int N = 16;
  while (trsm_cw_for(N + 16) != 0) N += 16;
  return N;
}
#define TRSM_DISPATCH_CW(cwv_, ...)                                 \
  switch (cwv_) {                                                   \
    case 16: { constexpr int CW = 16; __VA_ARGS__; } break;         \
    case 8: { constexpr int CW = 8; __VA_ARGS__; } break;           \
    case 4: { constexpr int CW = 4; __VA_ARGS__; } break;           \
    case 2: { constexpr int CW = 2; __VA_ARGS__; } break;           \
    default: { constexpr int CW = 1; __VA_ARGS__; } break;          \
  }

template <int CW>
__global__ void __launch_bounds__(64) k_trsm_fwd(int N, int K, int S, const double* __restrict__ Lall,
                                                 const double* __restrict__ Finv, const unsigned char* __restrict__ lchol,
                                                 double* __restrict__ Z) {
  extern __shared__ double lds[];
  const int cb = blockIdx.x, s = blockIdx.y, r = blockIdx.z, lane = threadIdx.x;
  if (!lchol[s]) return;
  const int Np = ((N + 15) >> 4) << 4;
  double* V = lds;
  double* P = V + (size_t)Np * (CW + 1);
  double* Zs = Z + ((size_t)r * S + s) * (size_t)K * N;
  trsm_slab_load<CW>(N, K, cb * CW, Zs, V, lane);
  trsm_fwd_wave<CW>(N, Lall + (size_t)s * N * N, Finv + (size_t)s * TRSM_NBLK(N) * 256, V, P, lane);
  trsm_slab_store<CW>(N, K, cb * CW, Zs, V, lane);
}

template <int CW>
__global__ void __launch_bounds__(64) k_trsm_bwd(int N, int K, int S, const double* __restrict__ Lall,
                                                 const double* __restrict__ Finv, const unsigned char* __restrict__ lchol,
                                                 const double* __restrict__ Vin, double* __restrict__ Xo) {
  extern __shared__ double lds[];
  const int cb = blockIdx.x, s = blockIdx.y, r = blockIdx.z, lane = threadIdx.x;
  if (!lchol[s]) return;
  const int Np = ((N + 15) >> 4) << 4;
  double* V = lds;
  trsm_slab_load<CW>(N, K, cb * CW, Vin + ((size_t)r * S + s) * (size_t)K * N, V, lane);
  trsm_bwd_wave<CW>(N, Lall + (size_t)s * N * N, Finv + (size_t)s * TRSM_NBLK(N) * 256, V, lane);
  trsm_slab_store<CW>(N, K, cb * CW, Xo + ((size_t)r * S + s) * (size_t)K * N, V, lane);
}

// host side: the slab solves with the slab width that fits N (one wave per CW columns, hyper-sample s, restart r)
template <bool BWD>
static inline hipError_t trsm2_launch(hipStream_t st, int N, int K, int S, int R, const double* Lall, const double* Finv,
                                      const unsigned char* lchol, const double* Zin, double* Zout);
static inline bool trsm2_wanted(int N);
static inline hipError_t trsm_fwd_launch(hipStream_t st, int N, int K, int S, int R, const double* Lall, const double* Finv,
                                         const unsigned char* lchol, double* Z) {
  if (trsm2_wanted(N)) return trsm2_launch<false>(st, N, K, S, R, Lall, Finv, lchol, Z, Z);
  const int cw = trsm_cw_for(N);
  if (cw == 0) return hipErrorInvalidValue;
  TRSM_DISPATCH_CW(cw, {
    const size_t lds = TRSM_LDS_BYTES_CW(N, CW);
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void*)k_trsm_fwd<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_trsm_fwd<CW>), dim3((K + CW - 1) / CW, S, R), dim3(64), lds, st, N, K, S, Lall, Finv, lchol, Z);
  });
  return hipGetLastError();
}
static inline hipError_t trsm_bwd_launch(hipStream_t st, int N, int K, int S, int R, const double* Lall, const double* Finv,
                                         const unsigned char* lchol, const double* Vin, double* Xo) {
  if (trsm2_wanted(N)) return trsm2_launch<true>(st, N, K, S, R, Lall, Finv, lchol, Vin, Xo);
  const int cw = trsm_cw_for(N);
  if (cw == 0) return hipErrorInvalidValue;
  TRSM_DISPATCH_CW(cw, {
    const size_t lds = TRSM_LDS_BYTES_CW(N, CW);
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void*)k_trsm_bwd<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_trsm_bwd<CW>), dim3((K + CW - 1) / CW, S, R), dim3(64), lds, st, N, K, S, Lall, Finv, lchol, Vin, Xo);
  });
  return hipGetLastError();
}
// k_spd_inverse: X = R^{-1} R^{-T} = inv(R'R) for the factors flagged in `on`, one wave per 16 columns of the identity:
// forward substitution from the column block's own rows (the slab is zero above them), backward substitution down to
// the same rows, i.e. the block column of the LOWER triangle, written together with its mirror image.  A third of the
// flops of two full-width solves on the identity, and no intermediate matrix in global memory.  Used for
// Kinv in the GP marginal-likelihood gradient (gplite_core.m:146-147) and for the stored -inv(K + sn2 I) of
// low-noise posteriors (gplite_core.m:84).
// T = inv(R') = R' \ I (lower triangular), one wave per 16 columns: the identity slab is formed in LDS and the substitution
// starts at the column block's own rows (everything above is zero and is written as such).
// transposed != 0 writes T' instead (row k of inv(R') contiguous: the operand layout k_syrk_tt wants).
template <int CW>
__global__ void __launch_bounds__(64) k_tri_inverse(int N, int S, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                    const unsigned char* __restrict__ lchol, double* __restrict__ T, int transposed) {
  extern __shared__ double lds[];
  const int cb = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  if (!lchol[s]) return;
  const int Np = ((N + 15) >> 4) << 4, k0 = cb * CW;
  double* V = lds;
  double* P = V + (size_t)Np * (CW + 1);
  for (int c = 0; c < CW; ++c)
    for (int i = lane; i < Np; i += 64) V[i * (CW + 1) + c] = (i == k0 + c && i < N) ? 1.0 : 0.0;
  trsm_wsync();
  trsm_fwd_wave<CW>(N, Lall + (size_t)s * N * N, Finv + (size_t)s * TRSM_NBLK(N) * 256, V, P, lane, k0 >> 4);
  if (!transposed) {
    trsm_slab_store<CW>(N, N, k0, T + (size_t)s * N * N, V, lane);
  } else {
    // TT[k][i] = T[k][i] at k * N + i: 64 / CW rows x CW consecutive columns per store; rows above the block are zero
    double* TT = T + (size_t)s * N * N;
    const int cc = lane % CW;
    if (k0 + cc < N)
      for (int k = lane / CW; k < N; k += 64 / CW) TT[(size_t)k * N + k0 + cc] = V[k * (CW + 1) + cc];
  }
}

// The same inverse, latency-shaped (round 5): ONE WORKGROUP of TRI2_W waves per 16-column slab instead of one wave, right-looking.
// The slab never touches LDS: wave w keeps the row blocks cb + w, cb + w + TRI2_W, ... of the right-hand side in accumulator
// registers (acc[slot]).  Per 16-row block step b
//   owner   (wave (b - cb) % TRI2_W): V_b = inv(R_bb') acc -- four MFMAs; register r of the accumulator layout is k-slice r of a
//           B operand, so the product needs no exchange --, V_b to LDS (double-buffered by step parity) and to global memory;
//   barrier (LDS only: the loads in flight for the next step are not waited for);
//   update  every wave, for each of its row blocks i > b: acc_i -= R[b, i]' V_b, four MFMAs; the tile R[b, i] (one 32-byte load
//           per lane: rows b0 + 4 lg .. + 3 of column i0 + li, the inner index permuted to match) was fetched a step ahead.
// The chain per step is two MFMA quadruples and one LDS round trip (~0.3 us) where the one-wave kernel walked a growing
// left-looking update behind every block (4.6 us per step at N = 400: 115 us for the first slab, the critical path of a
// gplite_nlZ gradient for one hyper-parameter vector).  Up to TRI2_W * MAXS row blocks below the slab's own.
#define TRI2_W 8
template <int MAXS, int DEPTH>
__device__ __forceinline__ void tri_inverse2_body(int N, int cb, int s, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                  double* __restrict__ T, int transposed) {
  static_assert(TRI2_W % DEPTH == 0, "the tile ring is indexed by the step modulo DEPTH");
  __shared__ double Vb[2][16 * 17];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = (N + 15) >> 4, k0 = cb << 4;
  const double* R = Lall + (size_t)s * N * N;
  const double* Fi = Finv + (size_t)s * nblk * 256;
  double* To = T + (size_t)s * N * N;
  typedef double d4u __attribute__((ext_vector_type(4), aligned(8)));
  // rows above the slab's own block are zero, and are written as such
  for (int e = tid; e < k0 * 16; e += 64 * TRI2_W) {
    const int k = e >> 4, c = k0 + (e & 15);
    if (c < N) To[transposed ? (size_t)k * N + c : (size_t)c * N + k] = 0.0;
  }
  tmf4 acc[MAXS];
  // Tiles R[b, i] of this wave's row blocks i > b (the A operand of the update, negated at use), fetched DEPTH steps ahead into a
  // ring: a step is ~0.4 us of dependent MFMAs and one LDS round trip, an L2 round trip ~1 us -- one step of look-ahead left every
  // step waiting for its tiles (1.3 us per step measured).
  tmf4 pre[DEPTH][MAXS];
#pragma unroll
  for (int sl = 0; sl < MAXS; ++sl) acc[sl] = (tmf4){0.0, 0.0, 0.0, 0.0};
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = (4 * r + lg == li) ? 1.0 : 0.0;       // the identity block
  }
  auto fetch = [&](int b, tmf4 (&pr)[MAXS]) {
#pragma unroll
    for (int sl = 0; sl < MAXS; ++sl) {
      const int i = cb + wave + TRI2_W * sl;                     // wave-uniform
      const int col = (i << 4) + li;
      tmf4 v = {0.0, 0.0, 0.0, 0.0};
      if (i > b && i < nblk && col < N) {                        // rows b0 .. b0 + 15 exist: b < i <= nblk - 1
        const d4u t = *reinterpret_cast<const d4u*>(R + (size_t)col * N + (b << 4) + 4 * lg);
        v = (tmf4){t[0], t[1], t[2], t[3]};
      }
      pr[sl] = v;
    }
  };
  double fv[4];      // this wave's next diagonal block inverse: A[i = li][k = 4u + lg] = Finv_b[li][4u + lg]
  auto fetch_fv = [&](int b) {
#pragma unroll
    for (int u = 0; u < 4; ++u) fv[u] = b < nblk ? Fi[(size_t)b * 256 + li * 16 + 4 * u + lg] : 0.0;
  };
  fetch_fv(cb + wave);
#pragma unroll
  for (int q = 0; q < DEPTH; ++q) fetch(cb + q, pre[q]);
  bool done = false;
#pragma unroll
  for (int sb = 0; sb < MAXS; ++sb) {
    for (int ow0 = 0; ow0 < TRI2_W && !done; ow0 += DEPTH) {
#pragma unroll
      for (int q = 0; q < DEPTH; ++q) {
        const int ow = ow0 + q;
        const int b = cb + sb * TRI2_W + ow, b0 = b << 4;
        if (b >= nblk) { done = true; }
        if (!done) {
          double* Vw = Vb[q & 1];                                // DEPTH is even: the parity of the step
          if (wave == ow) {
            tmf4 vb = {0.0, 0.0, 0.0, 0.0}, vb2 = {0.0, 0.0, 0.0, 0.0};
            vb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[0], acc[sb][0], vb, 0, 0, 0);
            vb2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[1], acc[sb][1], vb2, 0, 0, 0);
            vb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[2], acc[sb][2], vb, 0, 0, 0);
            vb2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[3], acc[sb][3], vb2, 0, 0, 0);
            vb += vb2;
#pragma unroll
            for (int r = 0; r < 4; ++r) Vw[(4 * r + lg) * 17 + li] = vb[r];
            const int c = k0 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = b0 + 4 * r + lg;
              if (k < N && c < N) To[transposed ? (size_t)k * N + c : (size_t)c * N + k] = vb[r];
            }
            fetch_fv(b + TRI2_W);
          }
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          if (b + 1 < nblk) {
            double bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) bv[u] = Vw[(4 * lg + u) * 17 + li];
#pragma unroll
            for (int sl = sb; sl < MAXS; ++sl) {
              const int i = cb + wave + TRI2_W * sl;
              if (i > b && i < nblk) {                           // wave-uniform
                tmf4 a2 = {0.0, 0.0, 0.0, 0.0};
                acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][0], bv[0], acc[sl], 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][1], bv[1], a2, 0, 0, 0);
                acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][2], bv[2], acc[sl], 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][3], bv[3], a2, 0, 0, 0);
                acc[sl] += a2;
              }
            }
            fetch(b + DEPTH, pre[q]);
          }
        }
      }
    }
  }
}

template <int MAXS>
__global__ void __launch_bounds__(64 * TRI2_W, 2) k_tri_inverse2(int N, int S, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                              const unsigned char* __restrict__ lchol, double* __restrict__ T, int transposed) {
  const int cb = blockIdx.x, s = blockIdx.y;
  if (!lchol[s]) return;
  tri_inverse2_body<MAXS, (MAXS <= 4 ? 4 : 2)>(N, cb, s, Lall, Finv, T, transposed);
}
static inline bool tri_inverse2_fits(int N) { return TRSM_NBLK(N) <= TRI2_W * 8; }

// The general slab solves in the same shape (round 5): R' V = Z (BWD = false) and R X = V (BWD = true) for 16 right-hand sides per
// workgroup of TRI2_W waves, the slab's row blocks in accumulator registers, V_b / X_b through a double-buffered 2 KB of LDS, tiles of
// R fetched DEPTH steps ahead.  Forward: blocks 0, 1, ... (wave w owns blocks w, w + 8, ...), update acc_i -= R[b, i]' V_b with the
// tile read as one 32-byte vector per lane (rows b0 + 4 lg .. + 3 of column i0 + li: the inner index permuted, the LDS read of V_b
// permuted to match).  Backward: blocks nblk - 1, nblk - 2, ... (wave w owns nblk - 1 - w, nblk - 9 - w, ...), update
// acc_i -= R[i, b] X_b with the tile's four columns 4 u + lg per lane (16 consecutive rows across li: one cache line per column),
// the block inverse transposed (R_bb^-1 = Finv_b').  Z is [r][s][k][N] (column k of the right-hand sides contiguous), in place or
// into Xo.  One-wave-per-slab kernels k_trsm_fwd / k_trsm_bwd: 144 / 178 us at N = 400 (5.8 / 7.1 us per block step).
template <int MAXS, int DEPTH, bool BWD>
__device__ __forceinline__ void trsm2_body(int N, int K, int k0, const double* __restrict__ R, const double* __restrict__ Fi,
                                           const double* __restrict__ Zin, double* __restrict__ Zout) {
  static_assert(TRI2_W % DEPTH == 0, "the tile ring is indexed by the step modulo DEPTH");
  __shared__ double Vb[2][16 * 17];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = (N + 15) >> 4;
  typedef double d4u __attribute__((ext_vector_type(4), aligned(8)));
  const int col = k0 + li;                                      // this lane's right-hand side
  tmf4 acc[MAXS], pre[DEPTH][MAXS];
  // step st = 0, 1, ... handles block blk(st) = st (forward) / nblk - 1 - st (backward); wave w owns the steps w, w + 8, ...
  auto blk = [&](int st) { return BWD ? nblk - 1 - st : st; };
#pragma unroll
  for (int sl = 0; sl < MAXS; ++sl) {
    const int st = wave + TRI2_W * sl, b = blk(st);
    tmf4 v = {0.0, 0.0, 0.0, 0.0};
    if (st < nblk && col < K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (b << 4) + 4 * r + lg;
        v[r] = row < N ? Zin[(size_t)col * N + row] : 0.0;
      }
    }
    acc[sl] = v;
  }
  // tiles for step st: the A operands of this wave's blocks still to come
  auto fetch = [&](int st, tmf4 (&pr)[MAXS]) {
    const int b = blk(st);
#pragma unroll
    for (int sl = 0; sl < MAXS; ++sl) {
      const int sti = wave + TRI2_W * sl, i = blk(sti);        // wave-uniform
      tmf4 v = {0.0, 0.0, 0.0, 0.0};
      if (sti > st && sti < nblk && st < nblk) {
        if (!BWD) {
          const int c = (i << 4) + li;                          // R[b0 + 4 lg + u][i0 + li], u = 0 .. 3 (block b is not the last: its rows exist)
          if (c < N) {
            const d4u t = *reinterpret_cast<const d4u*>(R + (size_t)c * N + (b << 4) + 4 * lg);
            v = (tmf4){t[0], t[1], t[2], t[3]};
          }
        } else {
          const int row = (i << 4) + li;                        // R[i0 + li][b0 + 4 u + lg], u = 0 .. 3 (block i is not the last: its rows exist)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = (b << 4) + 4 * u + lg;
            v[u] = c < N ? R[(size_t)c * N + row] : 0.0;
          }
        }
      }
      pr[sl] = v;
    }
  };
  double fv[4];      // block inverse as the A operand: forward Finv_b[li][k], backward Finv_b[k][li]
  auto fetch_fv = [&](int st) {
    const int b = blk(st);
#pragma unroll
    for (int u = 0; u < 4; ++u) fv[u] = st < nblk ? (BWD ? Fi[(size_t)b * 256 + (4 * u + lg) * 16 + li] : Fi[(size_t)b * 256 + li * 16 + 4 * u + lg]) : 0.0;
  };
  fetch_fv(wave);
#pragma unroll
  for (int q = 0; q < DEPTH; ++q) fetch(q, pre[q]);
  bool done = false;
#pragma unroll
  for (int sb = 0; sb < MAXS; ++sb) {
    for (int ow0 = 0; ow0 < TRI2_W && !done; ow0 += DEPTH) {
#pragma unroll
      for (int q = 0; q < DEPTH; ++q) {
        const int ow = ow0 + q;
        const int st = sb * TRI2_W + ow, b = blk(st), b0 = b << 4;
        if (st >= nblk) { done = true; }
        if (!done) {
          double* Vw = Vb[q & 1];                                // DEPTH is even: the parity of the step
          if (wave == ow) {
            tmf4 vb = {0.0, 0.0, 0.0, 0.0}, vb2 = {0.0, 0.0, 0.0, 0.0};
            vb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[0], acc[sb][0], vb, 0, 0, 0);
            vb2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[1], acc[sb][1], vb2, 0, 0, 0);
            vb = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[2], acc[sb][2], vb, 0, 0, 0);
            vb2 = __builtin_amdgcn_mfma_f64_16x16x4f64(fv[3], acc[sb][3], vb2, 0, 0, 0);
            vb += vb2;
#pragma unroll
            for (int r = 0; r < 4; ++r) Vw[(4 * r + lg) * 17 + li] = vb[r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = b0 + 4 * r + lg;
              if (row < N && col < K) Zout[(size_t)col * N + row] = vb[r];
            }
            fetch_fv(st + TRI2_W);
          }
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          if (st + 1 < nblk) {
            double bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) bv[u] = BWD ? Vw[(4 * u + lg) * 17 + li] : Vw[(4 * lg + u) * 17 + li];
#pragma unroll
            for (int sl = sb; sl < MAXS; ++sl) {
              const int sti = wave + TRI2_W * sl;
              if (sti > st && sti < nblk) {                      // wave-uniform
                tmf4 a2 = {0.0, 0.0, 0.0, 0.0};
                acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][0], bv[0], acc[sl], 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][1], bv[1], a2, 0, 0, 0);
                acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][2], bv[2], acc[sl], 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-pre[q][sl][3], bv[3], a2, 0, 0, 0);
                acc[sl] += a2;
              }
            }
            fetch(st + DEPTH, pre[q]);
          }
        }
      }
    }
  }
}
template <int MAXS, bool BWD>
__global__ void __launch_bounds__(64 * TRI2_W, 2) k_trsm2(int N, int K, int S, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                         const unsigned char* __restrict__ lchol, const double* __restrict__ Zin,
                                                         double* __restrict__ Zout) {
  const int cb = blockIdx.x, s = blockIdx.y, r = blockIdx.z;
  if (!lchol[s]) return;
  const size_t off = ((size_t)r * S + s) * (size_t)K * N;
  trsm2_body<MAXS, (MAXS <= 4 ? 4 : 2), BWD>(N, K, cb * 16, Lall + (size_t)s * N * N, Finv + (size_t)s * TRSM_NBLK(N) * 256, Zin + off, Zout + off);
}
// the workgroup-per-slab solves when the row blocks fit the accumulator registers (N <= 1024)
static inline bool trsm2_wanted(int N) { return TRSM_NBLK(N) <= TRI2_W * 8; }
// its row-block slots per wave: k_trsm2<4> up to N = 512, k_trsm2<8> beyond
static inline int trsm2_slots(int N) { return TRSM_NBLK(N) <= TRI2_W * 4 ? 4 : 8; }
// what trsm_fwd_launch / trsm_bwd_launch run at N, for the reporting hooks: (VBMC_VARSOLVE_TRSM2, slots) or (VBMC_VARSOLVE_SLAB, CW)
static inline void trsm_form_for(int N, int* kind, int* width) {
  if (trsm2_wanted(N)) { *kind = VBMC_VARSOLVE_TRSM2; *width = trsm2_slots(N); }
  else { *kind = VBMC_VARSOLVE_SLAB; *width = trsm_cw_for(N); }
}
template <bool BWD>
static inline hipError_t trsm2_launch(hipStream_t st, int N, int K, int S, int R, const double* Lall, const double* Finv,
                                      const unsigned char* lchol, const double* Zin, double* Zout) {
  const dim3 grid((K + 15) / 16, S, R);
  if (trsm2_slots(N) == 4) hipLaunchKernelGGL((k_trsm2<4, BWD>), grid, dim3(64 * TRI2_W), 0, st, N, K, S, Lall, Finv, lchol, Zin, Zout);
  else hipLaunchKernelGGL((k_trsm2<8, BWD>), grid, dim3(64 * TRI2_W), 0, st, N, K, S, Lall, Finv, lchol, Zin, Zout);
  return hipGetLastError();
}

// T = inv(R') (transposed != 0: its transpose), see k_tri_inverse
static inline hipError_t tri_inverse_launch(hipStream_t st, int N, int S, const double* Lall, const double* Finv,
                                            const unsigned char* lchol, double* T, int transposed) {
  const int cw = trsm_cw_for(N);
  if (cw == 0) return hipErrorInvalidValue;
  // the workgroup-per-slab kernel whenever the slab's row blocks fit its accumulator registers (N <= 1024) -- built for the latency
  // of a handful of matrices, it is also 17 % of a whole gplite_nlZ batch faster at 64 and 256 matrices (78 -> 91 k, 133 -> 157 k
  // evals/s: the one-wave kernel runs at a tenth of the matrix-pipe rate)
  {
    const int nblk = TRSM_NBLK(N);
    if (nblk <= TRI2_W * 8) {
      if (nblk <= TRI2_W * 4) hipLaunchKernelGGL((k_tri_inverse2<4>), dim3(nblk, S, 1), dim3(64 * TRI2_W), 0, st, N, S, Lall, Finv, lchol, T, transposed);
      else hipLaunchKernelGGL((k_tri_inverse2<8>), dim3(nblk, S, 1), dim3(64 * TRI2_W), 0, st, N, S, Lall, Finv, lchol, T, transposed);
      return hipGetLastError();
    }
  }
  TRSM_DISPATCH_CW(cw, {
    const size_t lds = TRSM_LDS_BYTES_CW(N, CW);
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void*)k_tri_inverse<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_tri_inverse<CW>), dim3((N + CW - 1) / CW, S, 1), dim3(64), lds, st, N, S, Lall, Finv, lchol, T, transposed);
  });
  return hipGetLastError();
}

// C = T'T for lower-triangular T given as TT[k][i] (row k contiguous): the 64 x 64 tiles on and above the diagonal (column j,
// row i at j * N + i; diagonal tiles in full): C[i][j] = sum_{k >= max(i, j)} TT[k][i] TT[k][j].  With T = inv(R') this is inv(R'R), the inverse the
// marginal-likelihood gradient contracts with (gplite_core.m:240), formed by a parallel rank-k update on the matrix cores
// instead of a second, sequential triangular solve.  One workgroup = 4 waves = a 64 x 64 tile (2 x 2 waves of 32 x 32);
// the roles of the MFMA operands are swapped (rows <-> j) so that the stores run along i.
// NT = 2: 64 x 64 per workgroup as above (throughput: many matrices).  NT = 1: 32 x 32 per workgroup, one 16 x 16 tile per
// wave -- for a handful of matrices the kernel is a chain of k-groups per workgroup, each an L2 round trip plus its MFMAs, and a
// quarter of the MFMAs per group on four times the workgroups shortens exactly that chain (30 -> 12 us for one matrix of order 400).
// FULLNEG: the whole symmetric matrix, negated (C = -T'T: gp.post(s).L = -inv(K + sn2 I) of a low-noise posterior, gplite_core.m:98),
// the tiles above the diagonal 64 x 64 blocks written a second time as their mirror image.
template <int NT, bool FULLNEG = false>
__global__ void __launch_bounds__(256) k_syrk_tt(int N, const double* __restrict__ TTall, const unsigned char* __restrict__ on,
                                                 double* __restrict__ Call) {
  constexpr int WT = 16 * NT;                              // rows / columns per wave
  const int ti = blockIdx.x, tj = blockIdx.y, s = blockIdx.z;
  const bool diag64 = (ti * 2 * WT) / 64 == (tj * 2 * WT) / 64;     // inside a 64 x 64 diagonal tile: formed in full (k_nlz_grad reads both triangles of those)
  if (!on[s] || (ti > tj && !diag64)) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
  const int i0 = ti * 2 * WT + WT * (wv & 1), j0 = tj * 2 * WT + WT * (wv >> 1);
  if (i0 >= N || j0 >= N) return;                      // sub-tile outside the matrix (diagonal tiles are formed in full)
  const double* TT = TTall + (size_t)s * N * N;
  double* C = Call + (size_t)s * N * N;
  tmf4 acc[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = (tmf4){0.0, 0.0, 0.0, 0.0};
  const int kmin = (j0 > i0 ? j0 : i0) & ~3;           // rows above max(i, j) hold zeros in one of the two factors
  int ia[NT], ja[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) { ia[u] = i0 + 16 * u + li; ja[u] = j0 + 16 * u + li; }
  // groups of SY_G k-steps: the operand loads of the next group are in flight during the MFMAs of this one
  constexpr int SY_G = 8;
  double ac[SY_G][NT], bc[SY_G][NT], an[SY_G][NT], bn[SY_G][NT];
  auto ldg = [&](int k0, double (*av)[NT], double (*bv)[NT]) {
#pragma unroll
    for (int g = 0; g < SY_G; ++g) {
      const int kk = k0 + 4 * g + lg;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        av[g][u] = (kk < N && ja[u] < N) ? TT[(size_t)kk * N + ja[u]] : 0.0;   // "A" operand: the j side (rows of the accumulator)
        bv[g][u] = (kk < N && ia[u] < N) ? TT[(size_t)kk * N + ia[u]] : 0.0;   // "B" operand: the i side (columns)
      }
    }
  };
  ldg(kmin, ac, bc);
  for (int k = kmin; k < N; k += 4 * SY_G) {
    if (k + 4 * SY_G < N) ldg(k + 4 * SY_G, an, bn);
#pragma unroll
    for (int g = 0; g < SY_G; ++g)
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[g][a], bc[g][b], acc[a][b], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < SY_G; ++g)
#pragma unroll
      for (int u = 0; u < NT; ++u) { ac[g][u] = an[g][u]; bc[g][u] = bn[g][u]; }
  }
  // acc[a][b]: row = j0 + 16a + lg + 4r, column = i0 + 16b + li
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 16 * a + lg + 4 * r, i = i0 + 16 * b + li;
        if (j < N && i < N && (diag64 || i <= j)) {
          const double v = FULLNEG ? -acc[a][b][r] : acc[a][b][r];
          C[(size_t)j * N + i] = v;
          if (FULLNEG && !diag64) C[(size_t)i * N + j] = v;
        }
      }
}
// C = T'T for S matrices on stream st (fullneg: C = -T'T, both triangles).  form: 0 chosen from the amount of work, 1 / 2 the tile
// form NT of k_syrk_tt (a caller whose results must not depend on its batch size fixes it)
static inline void syrk_tt_launch(hipStream_t st, int N, int S, const double* TT, const unsigned char* on, double* C, bool fullneg = false,
                                  int form = 0) {
  const int t64 = (N + 63) / 64, t32 = (N + 31) / 32;
  const bool small = form ? form == 1 : (size_t)S * t64 * (t64 + 1) / 2 <= 128;
  if (fullneg) {
    if (small) hipLaunchKernelGGL((k_syrk_tt<1, true>), dim3(t32, t32, S), dim3(256), 0, st, N, TT, on, C);
    else hipLaunchKernelGGL((k_syrk_tt<2, true>), dim3(t64, t64, S), dim3(256), 0, st, N, TT, on, C);
  } else {
    if (small) hipLaunchKernelGGL((k_syrk_tt<1, false>), dim3(t32, t32, S), dim3(256), 0, st, N, TT, on, C);
    else hipLaunchKernelGGL((k_syrk_tt<2, false>), dim3(t64, t64, S), dim3(256), 0, st, N, TT, on, C);
  }
}

// Two waves per workgroup take the column blocks cb and nblk-1-cb: a long and a short solve, so that every workgroup does
// the same work and the two slabs (rows from the block's own first row down) together need Np + 16 rows of LDS.
#define SPDINV_LDS_BYTES(N) ((size_t)((((((N) + 15) >> 4) << 4) + 16) * TR_VS + 2 * 64 * TR_VS) * sizeof(double))
__global__ void __launch_bounds__(128) k_spd_inverse(int N, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                    const unsigned char* __restrict__ on, double* __restrict__ Xo) {
  extern __shared__ double lds[];
  const int s = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!on[s]) return;
  const int nblk = (N + 15) >> 4, Np = nblk << 4;
  const bool paired = blockDim.x == 128;              // 64 threads: one column block per workgroup (N too large to pair)
  const int cb = wv == 0 ? (int)blockIdx.x : nblk - 1 - (int)blockIdx.x;
  if (wv == 1 && cb == (int)blockIdx.x) return;       // odd block count: the middle block is done by wave 0
  const int k0 = cb << 4;
  // wave 0's slab holds rows k0 .. Np-1 at the start of the buffer, wave 1's (shorter) slab follows it
  double* Vbase = wv == 0 ? lds : lds + (size_t)(Np - ((int)blockIdx.x << 4)) * TR_VS;
  double* V = Vbase - (size_t)k0 * TR_VS;              // indexed by absolute row; rows < k0 are never touched
  double* P = lds + (size_t)(paired ? Np + 16 : Np) * TR_VS + (size_t)wv * 64 * TR_VS;
  for (int c = 0; c < 16; ++c)
    for (int i = k0 + lane; i < Np; i += 64) V[i * TR_VS + c] = (i == k0 + c && i < N) ? 1.0 : 0.0;
  trsm_wsync();
  const double* Rm = Lall + (size_t)s * N * N;
  const double* Fi = Finv + (size_t)s * TRSM_NBLK(N) * 256;
  trsm_fwd_wave<16>(N, Rm, Fi, V, P, lane, cb);
  trsm_bwd_wave<16>(N, Rm, Fi, V, lane, cb);
  double* X = Xo + (size_t)s * N * N;
  // columns of the block: rows from the block's own first row down (the diagonal block as computed, both halves)
  for (int c = 0; c < 16; ++c) {
    const int j = k0 + c;
    if (j >= N) break;
    for (int i = k0 + lane; i < N; i += 64) X[(size_t)j * N + i] = V[i * TR_VS + c];
  }
  // mirror image of the part below the diagonal block: 4 rows x 16 consecutive columns per store
  const int cc = lane & 15;
  if (k0 + cc < N)
    for (int i = k0 + 16 + (lane >> 4); i < N; i += 4) X[(size_t)(k0 + cc) + (size_t)i * N] = V[i * TR_VS + cc];
}

// Narrow-slab variant for N beyond the 16-column slab (see trsm_vld): one wave per CW columns of the identity, full-height slab.
// Element (i, j) of the symmetric inverse with i >= j is written by the slab of column j, together with its mirror image.
template <int CW>
__global__ void __launch_bounds__(64) k_spd_inverse_narrow(int N, const double* __restrict__ Lall, const double* __restrict__ Finv,
                                                           const unsigned char* __restrict__ on, double* __restrict__ Xo) {
  extern __shared__ double lds[];
  const int cb = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  if (!on[s]) return;
  const int Np = ((N + 15) >> 4) << 4, k0 = cb * CW, bi0 = k0 >> 4;
  double* V = lds;
  double* P = V + (size_t)Np * (CW + 1);
  for (int c = 0; c < CW; ++c)
    for (int i = lane; i < Np; i += 64) V[i * (CW + 1) + c] = (i == k0 + c && i < N) ? 1.0 : 0.0;
  trsm_wsync();
  const double* Rm = Lall + (size_t)s * N * N;
  const double* Fi = Finv + (size_t)s * TRSM_NBLK(N) * 256;
  trsm_fwd_wave<CW>(N, Rm, Fi, V, P, lane, bi0);
  trsm_bwd_wave<CW>(N, Rm, Fi, V, lane, bi0);
  double* X = Xo + (size_t)s * N * N;
  for (int c = 0; c < CW; ++c) {
    const int j = k0 + c;
    if (j >= N) break;
    for (int i = j + lane; i < N; i += 64) {
      const double v = V[i * (CW + 1) + c];
      X[(size_t)j * N + i] = v;
      if (i > j) X[(size_t)i * N + j] = v;
    }
  }
}

// host side: pick the paired launch when its LDS fits, else one column block per workgroup; narrow slabs beyond N = 1136
#define SPD_INVERSE_LAUNCH(ctx_, N_, S_, st_, Lall_, Finv_, on_, Xo_)                                                         \
  do {                                                                                                                        \
    const int cwv_ = trsm_cw_for(N_);                                                                                         \
    if (cwv_ != 16) {                                                                                                         \
      TRSM_DISPATCH_CW(cwv_, {                                                                                                \
        const size_t nl_ = TRSM_LDS_BYTES_CW(N_, CW);                                                                         \
        HIP_TRY(ctx_, hipFuncSetAttribute((const void*)k_spd_inverse_narrow<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)nl_)); \
        hipLaunchKernelGGL((k_spd_inverse_narrow<CW>), dim3(((N_) + CW - 1) / CW, S_), dim3(64), nl_, st_, N_, Lall_, Finv_, on_, Xo_); \
      });                                                                                                                     \
      break;                                                                                                                  \
    }                                                                                                                         \
    const bool pair_ = SPDINV_LDS_BYTES(N_) <= 160 * 1024;                                                                    \
    const size_t il_ = pair_ ? SPDINV_LDS_BYTES(N_) : TRSM_LDS_BYTES(N_);                                                     \
    if (il_ > 64 * 1024)                                                                                                      \
      HIP_TRY(ctx_, hipFuncSetAttribute((const void*)k_spd_inverse, hipFuncAttributeMaxDynamicSharedMemorySize, (int)il_));   \
    hipLaunchKernelGGL(k_spd_inverse, dim3(pair_ ? (TRSM_NBLK(N_) + 1) / 2 : TRSM_NBLK(N_), S_), dim3(pair_ ? 128 : 64), il_, st_, \
                       N_, Lall_, Finv_, on_, Xo_);                                                                           \
  } while (0)

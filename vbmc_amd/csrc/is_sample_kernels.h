// Device-resident MCMC of the IMIQR importance sampler (private/activeimportancesampling_vbmc.m:153-235, Step 2): per GP hyper-sample an
// ensemble slice sampler -- vbmc_amd/acq.py::ensemble_slice_sample, which stands in for the third-party eissample_lite.m -- on the target
//   logp(x) = ymu + u ys + log1p(-exp(-2 u ys)),  ys = sqrt(max(ys2, realmin)),  u = 0.6745        (acq/acqimiqr_vbmc.m:22-25)
// with [ymu, ys2] the prediction of the ensemble's OWN hyper-sample.  All randomness comes from an indexed uniform block
//   U[slot + 64 (j + H (e + S m))]   m: half-move, e: ensemble, j: position inside the moving half
//   slot 0: a = floor(u H)   1: b = (a + 1 + floor(u (H - 1))) mod H   2: level y = logp(x) + log u   3: L = -u, R = L + 1
//   slot 4 + q: q-th shrink proposal t = L + u (R - L); a rejected t < 0 becomes L, otherwise R
// so that the chain is a function of the block alone.  One ROUND is
//   k_is_step   one workgroup (one wave) per ensemble: consume the previous round's values in candidate order (an end of the stepping
//               out stops at the first step below the level, the shrinkage accepts the first proposal above it), commit a finished
//               half-move and record walkers, set up the next half-move, write this round's candidates -- up to 2 spec per walker while
//               stepping out, spec while shrinking -- and their in-bounds mask into the prediction's point buffer
//   k_is_pred   grid (16-point tiles of an ensemble's candidates, S): fmu, fs2, ys2 and the target of every candidate under its own
//               hyper-sample
// The ensembles are independent state machines: they need not advance in lock-step.  The left end after k steps is L0 - k, the right end
// R0 + k, a candidate is x + t v with every operation rounded on its own (contraction off, slice_prop), so a candidate has the same bits
// for every spec; a point's value depends neither on its slot nor on its companions (an MFMA output element is a function of its own row
// and column, every sum runs in a fixed order, nothing is atomic).
#pragma once
#include "common.h"
#include "dev_layout.h"
#include "device_math.h"
#include "gp_factor_kernels.h"   // gp_meanfun
#include "gp_pred_kernels.h"     // PredArgs
#include "parity_rng.h"          // srch_log, slice_uniform, slice_prop

#define IS_MAXH 33              // W = 2 H <= 2 (VBMC_LIM_D + 1)
#define IS_MAXSPEC 4
#define IS_MAXSTEPS 20
#define IS_MAXSHRINK 60
#define IS_SLOTS 64             // uniforms per walker and half-move: 4 + IS_MAXSHRINK
#define IS_MAXCAND (2 * IS_MAXSPEC * IS_MAXH)
static_assert(IS_MAXH == VBMC_LIM_D + 1 && 4 + IS_MAXSHRINK == IS_SLOTS && IS_MAXH <= 64, "one lane per walker of the moving half");
enum { IS_ERR_NONE = 0, IS_ERR_START = 1, IS_ERR_UNIFORMS = 2 };

struct IsEnsState {             // one per ensemble; the S of them are the progress words the host reads one chunk behind
  int done;                     // 1: Nm walkers recorded, or an error; later launches do nothing
  int err;                      // IS_ERR_*
  int init;                     // 0: nothing yet, 1: the starting walkers wait for their values, 2: running
  int m;                        // the half-move in progress, counted from 0: half m mod 2 moves
  int moved, nrec;              // walker moves committed, walkers recorded
  int ncand;                    // candidates of this round (what k_is_pred evaluates)
  int rounds, behind;           // launches that did work / that found the chain finished
  int pad_;
  long long funccount;          // in-bounds evaluations the one-at-a-time procedure consumes
  long long performed;          // in-bounds evaluations launched
};

struct IsWalker {               // one per position of the moving half
  int ph;                       // 0 stepping out, 1 shrinking, 2 done
  int kL, kR, gL, gR;           // unit steps inside the slice so far, ends still growing
  int steps, shr;               // rounds of steps / proposals consumed
  int a, b;                     // the direction's two walkers of the complementary half
  int nc, base;                 // this round's candidates: count and first slot
  int pad_;
  double y, L0, Lq, Rq;         // level, the placement L0 = -u, the shrinking interval
};

struct IsStepArgs {
  int D, S, W, H, Nm, thin, burnin, spec, max_steps, max_shrink, parity, Mmax, C;
  unsigned long long seed;
  const double *LB, *UB;        // D each
  const double* U;              // parity: IS_SLOTS x H x S x Mmax
  IsEnsState* st;               // S
  IsWalker* wk;                 // S x IS_MAXH
  double* x;                    // S x W x D: walker w of ensemble e at (e W + w) D
  double* lp;                   // S x W
  double* P;                    // S x D x C: the prediction's point buffer, candidate c of ensemble e at (e D + d) C + c
  unsigned char* mask;          // S x C: inside [LB, UB]
  const double* val;            // S x C: the target at last round's candidates (k_is_pred)
  double* Xa;                   // Nm x D x S recorded walkers
  double* rlp;                  // S x Nm: the chain's own value at each
};

// The sampler's block of fp64 state, from the shape alone (E ensembles, C candidates a round; nU: the parity uniforms, 0 without):
//   LB | UB | x | lp | P | val | the target's | Xa | rlp | U      (fixed: the bytes in front of U, zeroed at the start)
// The target describes its own region behind the values as a layout; its windows resolve against extra.at(block).
struct IsCoreBlock {
  DevLayout w;
  size_t fixed = 0;
  DevWin<double> LB, UB, x, lp, P, val, Xa, rlp, U;
  DevWin<unsigned char> extra;
  IsCoreBlock() {}
  IsCoreBlock(int D, int E, int W, int C, int Nm, const DevLayout& target, size_t nU) {
    LB = w.add<double>(D); UB = w.add<double>(D); x = w.add<double>((size_t)E * W * D); lp = w.add<double>((size_t)E * W);
    P = w.add<double>((size_t)E * D * C); val = w.add<double>((size_t)E * C); extra = w.add(target);
    Xa = w.add<double>((size_t)Nm * D * E); rlp = w.add<double>((size_t)E * Nm);
    fixed = w.bytes();
    U = w.add_if<double>(nU != 0, nU);
  }
  void bind(IsStepArgs& a, void* dw) const {
    a.LB = LB.at(dw); a.UB = UB.at(dw); a.x = x.at(dw); a.lp = lp.at(dw); a.P = P.at(dw); a.val = val.at(dw);
    a.Xa = Xa.at(dw); a.rlp = rlp.at(dw); a.U = U.at(dw);
  }
};

__device__ __forceinline__ double is_u(const IsStepArgs& a, int m, int e, int j, int slot) {
  if (!a.parity) return slice_uniform(a.seed, (unsigned)m, (unsigned)(e * a.H + j), (unsigned)slot);
  return a.U[(size_t)slot + IS_SLOTS * ((size_t)j + (size_t)a.H * ((size_t)e + (size_t)a.S * m))];
}
// the two ends after k unit steps and a point on the direction, every operation rounded on its own: shared by proposing and consuming
__device__ __forceinline__ double is_left(double L0, int k) {
#pragma clang fp contract(off)
  return L0 - (double)k;
}
__device__ __forceinline__ double is_right(double L0, int k) {
#pragma clang fp contract(off)
  return (L0 + 1.0) + (double)k;
}
__device__ __forceinline__ double is_point(double x, double t, double v) {
#pragma clang fp contract(off)
  return x + t * v;
}
// ln(1 - e) for 0 < e <= 1 from exactly rounded operations and the search's logarithm alone: with w = fl(1 - e) the quotient
// ln(w) / (w - 1) is smooth at 1, so ln(w) (-e) / (w - 1) carries the rounding of w away (Kahan's log1p); w = 1: -e, w = 0: -Inf
__device__ __forceinline__ double is_log1m(double e) {
#pragma clang fp contract(off)
  const double w = 1.0 - e;
  if (w == 1.0) return -e;
  if (!(w > 0.0)) return -__builtin_inf();
  return srch_log(w) * (-e) / (w - 1.0);
}

__global__ void __launch_bounds__(64) k_is_step(IsStepArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_cj[IS_MAXCAND];
  __shared__ double s_ct[IS_MAXCAND];
  __shared__ int s_nc[64];
  const int e = blockIdx.x, lane = threadIdx.x, D = a.D, W = a.W, H = a.H, C = a.C;
  IsEnsState* st = a.st + e;
  if (st->done) {
    if (lane == 0) st->behind = st->behind + 1;
    return;
  }
  IsWalker* wk = a.wk + (size_t)e * IS_MAXH;
  double* x = a.x + (size_t)e * W * D;
  double* lp = a.lp + (size_t)e * W;
  double* P = a.P + (size_t)e * D * C;
  unsigned char* mask = a.mask + (size_t)e * C;
  const double* val = a.val + (size_t)e * C;
  const double ninf = -__builtin_inf();
  const int init = st->init;
  if (init == 0) {                                   // the W starting walkers (inside the box: the host checked)
    for (int idx = lane; idx < W * D; idx += 64) { const int w = idx / D, d = idx % D; P[(size_t)d * C + w] = x[(size_t)w * D + d]; }
    for (int w = lane; w < W; w += 64) mask[w] = 1;
    if (lane == 0) { st->init = 1; st->ncand = W; st->rounds = st->rounds + 1; }
    return;
  }
  int m = st->m, moved = st->moved, nrec = st->nrec;
  long long funccount = st->funccount, performed = st->performed;
  bool setup = false;
  if (init == 1) {
    bool bad = false;
    for (int w = lane; w < W; w += 64) { const double v = val[w]; lp[w] = v; bad |= !(v > ninf && v < __builtin_inf()); }
    funccount += W; performed += W;
    if (__ballot(bad) != 0ull) {
      if (lane == 0) { st->err = IS_ERR_START; st->done = 1; st->ncand = 0; st->funccount = funccount; st->performed = performed; st->rounds = st->rounds + 1; }
      return;
    }
    m = 0;
    setup = true;
  } else {
    // ---- consume the previous round's values, candidate by candidate
    const int mine = (m & 1) * H + lane;
    int cf = 0, cp = 0;
    if (lane < H && wk[lane].ph < 2) {
      IsWalker w = wk[lane];
      const int base = w.base;
      if (w.ph == 0) {
        const int ns = min(a.spec, a.max_steps - w.steps);
        int c = 0;
        if (w.gL) {
          bool ok = true;
          for (int q = 0; q < ns; ++q, ++c) {
            const bool inb = mask[base + c] != 0;
            const double v = inb ? val[base + c] : ninf;
            cp += inb;
            if (!ok) continue;
            cf += inb;
            if (v > w.y) w.kL += 1; else { ok = false; w.gL = 0; }
          }
        }
        if (w.gR) {
          bool ok = true;
          for (int q = 0; q < ns; ++q, ++c) {
            const bool inb = mask[base + c] != 0;
            const double v = inb ? val[base + c] : ninf;
            cp += inb;
            if (!ok) continue;
            cf += inb;
            if (v > w.y) w.kR += 1; else { ok = false; w.gR = 0; }
          }
        }
        w.steps += ns;
        if (w.steps >= a.max_steps || (!w.gL && !w.gR)) { w.ph = 1; w.shr = 0; w.Lq = is_left(w.L0, w.kL); w.Rq = is_right(w.L0, w.kR); }
      } else {
        const int ns = min(a.spec, a.max_shrink - w.shr);
        bool acc = false;
        for (int q = 0; q < ns; ++q) {
          const bool inb = mask[base + q] != 0;
          const double v = inb ? val[base + q] : ninf;
          cp += inb;
          if (acc) continue;
          cf += inb;
          const double t = slice_prop(is_u(a, m, e, lane, 4 + w.shr + q), w.Lq, w.Rq);
          if (v > w.y) {
            acc = true;
            for (int d = 0; d < D; ++d) x[(size_t)mine * D + d] = P[(size_t)d * C + base + q];
            lp[mine] = v;
          } else if (t < 0.0) w.Lq = t;
          else w.Rq = t;
        }
        w.shr += ns;
        if (acc || w.shr >= a.max_shrink) w.ph = 2;   // (a walker whose slice collapsed stays where it is)
      }
      wk[lane] = w;
    }
    for (int o = 32; o > 0; o >>= 1) { cf += __shfl_xor(cf, o, 64); cp += __shfl_xor(cp, o, 64); }
    funccount += cf; performed += cp;
    __syncthreads();
    const bool open = lane < H && wk[lane].ph < 2;
    if (__ballot(open) == 0ull) {
      // ---- the half-move is finished: record by the host sampler's rule (one count per walker move, every thin-th after the burn-in)
      const int mv = moved + lane + 1;
      const bool rec = lane < H && mv > a.burnin && (mv - a.burnin) % a.thin == 0;
      const unsigned long long mr = __ballot(rec);
      const int ir = nrec + __popcll(mr & ((1ull << lane) - 1ull));
      if (rec && ir < a.Nm) {
        for (int d = 0; d < D; ++d) a.Xa[(size_t)ir + (size_t)a.Nm * (d + (size_t)D * e)] = x[(size_t)mine * D + d];
        a.rlp[(size_t)e * a.Nm + ir] = lp[mine];
      }
      nrec = min(a.Nm, nrec + __popcll(mr));
      moved += H;
      m += 1;
      if (nrec >= a.Nm) {
        if (lane == 0) { st->done = 1; st->ncand = 0; st->m = m; st->moved = moved; st->nrec = nrec; st->funccount = funccount; st->performed = performed; st->rounds = st->rounds + 1; }
        return;
      }
      setup = true;
    }
  }
  if (setup) {
    if (a.parity && m >= a.Mmax) {
      if (lane == 0) { st->err = IS_ERR_UNIFORMS; st->done = 1; st->ncand = 0; st->init = 2; st->m = m; st->moved = moved; st->nrec = nrec; st->funccount = funccount; st->performed = performed; st->rounds = st->rounds + 1; }
      return;
    }
    __syncthreads();
    if (lane < H) {
      IsWalker w{};
      const double u0 = is_u(a, m, e, lane, 0), u1 = is_u(a, m, e, lane, 1), u2 = is_u(a, m, e, lane, 2), u3 = is_u(a, m, e, lane, 3);
      w.a = min((int)floor(u0 * (double)H), H - 1);
      w.b = (w.a + 1 + min((int)floor(u1 * (double)(H - 1)), H - 2)) % H;
      w.y = lp[(m & 1) * H + lane] + srch_log(u2);
      w.L0 = -u3;
      w.gL = 1; w.gR = 1;
      wk[lane] = w;
    }
  }
  __syncthreads();
  // ---- this round's candidates: slots in walker order, left steps before right steps
  {
    int nc = 0;
    if (lane < H) {
      const IsWalker w = wk[lane];
      if (w.ph == 0) nc = min(a.spec, a.max_steps - w.steps) * (w.gL + w.gR);
      else if (w.ph == 1) nc = min(a.spec, a.max_shrink - w.shr);
    }
    s_nc[lane] = nc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int j = 0; j < H; ++j) { const int n = s_nc[j]; if (j < lane) base += n; tot += n; }
    if (lane < H && nc > 0) {
      IsWalker w = wk[lane];
      w.nc = nc; w.base = base;
      int c = base;
      if (w.ph == 0) {
        const int ns = min(a.spec, a.max_steps - w.steps);
        if (w.gL) for (int q = 0; q < ns; ++q, ++c) { s_cj[c] = lane; s_ct[c] = is_left(w.L0, w.kL + q); }
        if (w.gR) for (int q = 0; q < ns; ++q, ++c) { s_cj[c] = lane; s_ct[c] = is_right(w.L0, w.kR + q); }
      } else {
        double Lq = w.Lq, Rq = w.Rq;
        for (int q = 0; q < nc; ++q, ++c) {
          const double t = slice_prop(is_u(a, m, e, lane, 4 + w.shr + q), Lq, Rq);
          s_cj[c] = lane; s_ct[c] = t;
          if (t < 0.0) Lq = t; else Rq = t;
        }
      }
      wk[lane] = w;
    }
    __syncthreads();
    const int hm = (m & 1) * H, ho = H - hm;          // first walker of the moving half, of the complementary half
    for (int c = lane; c < tot; c += 64) {
      const int j = s_cj[c];
      const double t = s_ct[c];
      const double* xc = x + (size_t)(hm + j) * D;
      const double* xa = x + (size_t)(ho + wk[j].a) * D;
      const double* xb = x + (size_t)(ho + wk[j].b) * D;
      bool inb = true;
      for (int d = 0; d < D; ++d) {
        const double p = is_point(xc[d], t, xb[d] - xa[d]);
        P[(size_t)d * C + c] = p;
        inb = inb && p >= a.LB[d] && p <= a.UB[d];
      }
      mask[c] = inb ? 1 : 0;
    }
    if (lane == 0) {
      st->init = 2; st->m = m; st->moved = moved; st->nrec = nrec; st->ncand = tot;
      st->funccount = funccount; st->performed = performed; st->rounds = st->rounds + 1;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_is_pred: gplite_pred (gplite_pred.m:73-121) of candidate c of ensemble s under hyper-sample s ALONE, and the target.  One workgroup
// per (16-point tile, s): its waves compute the sW-scaled N x 16 cross-kernel tile once, into LDS (the distances as QS MFMAs per
// 16 x 16 block, inner dimension D, and the table exponential, as k_pred_ks), Ks' alpha on the way; they then walk the 16-row tiles of
// inv(L') against the LDS tile -- dealt in snake order, descending cost -- and the sums of squares are added per wave in tile order, then
// in wave order.  Lchol = false: all columns of L, the sum of Ks .* (L Ks).  Points beyond ncand[s] and masked points are skipped.
#define ISP_THREADS 512
#define ISP_LDS_BYTES(NP_) ((size_t)(NP_) * 16 * sizeof(double))
struct IsPredArgs {
  PredArgs pa;                  // the GP (Xs, mean_b, fmu, fs2, ys2 are not read)
  const double *Xc, *aa, *muv;  // k_pred_prep's per-hyper-sample set-up with mc = 0
  const double* P;              // S x D x C
  const unsigned char* mask;    // S x C or null
  const int* ncand;             // candidates of ensemble e at ncand[e * nstride]  (k_is_pred: e = s)
  int nstride, C;
  double *logp, *fmu, *fs2, *ys2;   // S x C each
};

// The body of k_is_pred and of k_gs_pred (gp_surrogate_kernels.h): the points of ensemble e under hyper-sample s.  SURR = false: e = s,
// the four outputs at [s][c] and the IMIQR target.  SURR = true: ymu (= fmu) and ys2 at [s][e][c] of E ensembles, no target.
template <int QS, bool SURR>
__device__ __forceinline__ void isp_body(const IsPredArgs& g, const int t, const int e, const int s, const int E) {
  constexpr int NWV = ISP_THREADS / 64;
  extern __shared__ double KsL[];              // [n][16], sW-scaled, zero for n >= N and for skipped points
  __shared__ double tab[VB_EXP_TAB_N];
  __shared__ double WS[NWV][16];               // per-wave sums: Ks' alpha first, the variance's sum afterwards
  const PredArgs& a = g.pa;
  const int C = g.C;
  const int nc = min(g.ncand[(size_t)e * g.nstride], C);
  if (16 * t >= nc) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int jc = 16 * t + li;
  const bool cv = jc < nc && (!g.mask || g.mask[(size_t)e * C + jc] != 0);
  if (__ballot(cv) == 0ull) return;            // (every wave sees the same sixteen points)
  const int N = a.N, D = a.D, Np = ((N + 15) >> 4) << 4, nblk = Np >> 4;
  for (int i = tid; i < VB_EXP_TAB_N; i += ISP_THREADS) tab[i] = c_exp2_tab[i];
  __syncthreads();
  const double* h = a.hyp + (size_t)s * a.Nhyp;
  const double* mu = g.muv + (size_t)s * 2 * D;
  const double* iell = mu + D;
  const double lsf2 = 2.0 * h[D];
  const bool lc = a.lchol[s] != 0;
  const double sW = lc ? 1.0 / sqrt(a.sn2_eff[s]) : 1.0;
  const double* xcs = g.Xc + (size_t)s * N * D;
  const double* aas = g.aa + (size_t)s * N;
  const double* al = a.alpha + (size_t)s * N;
  const double* Ps = g.P + (size_t)e * D * C;
  // ---- the cross-kernel tile: wave w takes the row blocks w, w + NWV, ...
  double xb[QS], bb = 0.0, fmacc = 0.0;
#pragma unroll
  for (int q = 0; q < QS; ++q) {
    const int d = 4 * q + lg;
    xb[q] = (cv && d < D) ? fma(Ps[(size_t)d * C + jc], iell[d], -mu[d]) : 0.0;
    bb = fma(xb[q], xb[q], bb);
  }
  bb = xor_sum16(bb);
  bb = xor_sum32(bb);
  for (int nb = wave; nb < nblk; nb += NWV) {
    const int n0 = nb * 16, na = min(n0 + li, N - 1);
    vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int d = 4 * q + lg;
      const double av = d < D ? xcs[(size_t)na * D + d] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xb[q], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + lg + 4 * r;
      double v = 0.0;
      if (n < N && cv) {
        const double cdist = fmax(aas[n] + (bb - 2.0 * acc[r]), 0.0);      // sq_dist.m:45,49
        v = vb_exp_tab<0>(lsf2 - cdist / 2.0, tab);                        // sf2 exp(-K/2)  (gplite_pred.m:74)
        fmacc = fma(v, al[n], fmacc);
      }
      KsL[(size_t)(n0 + lg + 4 * r) * 16 + li] = v * sW;                   // sW .* Ks  (:99)
    }
  }
  fmacc = xor_sum16(fmacc);
  fmacc = xor_sum32(fmacc);
  if (lg == 0) WS[wave][li] = fmacc;
  __syncthreads();
  double fm = 0.0;
  if (tid < 16)
    for (int w = 0; w < NWV; ++w) fm += WS[w][tid];
  // ---- the product: this wave's row tiles of inv(L') (or of L) against the resident tile
  const double* Am = (lc ? a.tinv : a.L) + (size_t)s * N * N;   // element (row, col) at col * N + row
  double part = 0.0;
  for (int k = 0; k < nblk; ++k) {
    const int kr = k % (2 * NWV);
    if ((kr < NWV ? kr : 2 * NWV - 1 - kr) != wave) continue;
    const int rt = nblk - 1 - k;
    const int ncol = lc ? (rt + 1) * 16 : Np;
    const int row = rt * 16 + li;
    vb_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < ncol; c0 += 16) {      // (ncol is a multiple of 16: four k-steps, their loads ahead of the MFMAs)
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int col = c0 + 4 * u + lg;
        av[u] = (row < N && col < N) ? Am[(size_t)col * N + row] : 0.0;
        bv[u] = KsL[(size_t)col * 16 + li];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
    // C layout: lane (col = li = point, row = rt * 16 + lg + 4 q)
    if (lc) {
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fma(acc[q], acc[q], part);                                   // sum(V .* V)          (:100)
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fma(KsL[(size_t)(rt * 16 + lg + 4 * q) * 16 + li], acc[q], part);   // sum(Ks .* (L * Ks))  (:104)
    }
  }
  part = xor_sum16(part);
  part = xor_sum32(part);
  __syncthreads();                             // (Ks' alpha has been read)
  if (lg == 0) WS[wave][li] = part;
  __syncthreads();
  if (tid >= 16 || !cv) return;
  double pv = 0.0;
  for (int w = 0; w < NWV; ++w) pv += WS[w][tid];
  // ---- fmu = m* + Ks' alpha (:83), fs2 = max(kss -/+ pv, 0) (:100,:104,:120), ys2 (:121; no s2star, no ystar), the target
  const double sf2 = vb_exp_tab<0>(2.0 * h[D], tab);
  const double fmu = gp_meanfun(a.meanfun, D, h + a.moff, Ps + jc, (size_t)C) + fm;
  const double fs2 = fmax(lc ? sf2 - pv : sf2 + pv, 0.0);
  const double sn2s = a.nf0 ? vb_exp_tab<0>(2.0 * h[a.noff], tab) : 2.220446049250313e-16;
  const double ys2 = fs2 + sn2s * a.sn2_mult[s];
  if (SURR) {
    const size_t o = ((size_t)s * E + e) * C + jc;
    g.fmu[o] = fmu; g.ys2[o] = ys2;
    return;
  }
  const double u = 0.6745;
  const double ys = sqrt(fmax(ys2, 2.2250738585072014e-308));
  double lp = fmu + (u * ys + is_log1m(vb_exp_tab<0>(-2.0 * u * ys, tab)));     // (the library's table exponential and logarithm)
  if (!(lp > -__builtin_inf() && lp < __builtin_inf())) lp = -__builtin_inf();
  const size_t o = (size_t)s * C + jc;
  g.logp[o] = lp; g.fmu[o] = fmu; g.fs2[o] = fs2; g.ys2[o] = ys2;
}

template <int QS>
__global__ void __launch_bounds__(ISP_THREADS) k_is_pred(IsPredArgs g) {
  isp_body<QS, false>(g, blockIdx.x, blockIdx.y, blockIdx.y, 0);
}

// lnw = fmu - logp and fs2a of the recorded walkers in the layout of the importance-sampling state (S x Nap, -inf / 0 in the padding)
__global__ void __launch_bounds__(256) k_is_finish(int S, int Nm, int Nap, const double* __restrict__ fmu, const double* __restrict__ fs2,
                                                   const double* __restrict__ rlp, double* __restrict__ lnw, double* __restrict__ fs2a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * Nap) return;
  const int s = i / Nap, c = i % Nap;
  lnw[i] = c < Nm ? fmu[(size_t)s * Nm + c] - rlp[(size_t)s * Nm + c] : -__builtin_inf();
  fs2a[i] = c < Nm ? fs2[(size_t)s * Nm + c] : 0.0;
}

// Device-resident slice sampler for the GP hyper-parameter posterior (utils/slicesamplebnd.m:229-358 with StepOut = false, target
// gp_objfun with swapsign, gplite_train.m:318): the chain's state lives on the device and one ROUND of the chain is
//   k_slice_propose  W speculative shrink proposals of the open coordinate -> the hyper-parameter block, noise vectors, jitter scalars
//                    and hyper-prior of the batched gplite_nlZ value path (k_gp_scale .. k_nlz_final, gp_factor.h: gp_launch_*)
//   k_slice_decide   first accepted proposal (in order), chain update, bookkeeping of a finished sweep, set-up of the next coordinate
// Speculation: with StepOut = false the k-th proposal UNDER THE HYPOTHESIS that proposals 1 .. k-1 were rejected is a function of the
// current point, the interval and the uniforms alone (:283-304: a rejection moves the interval's end on the proposal's side).  Both
// kernels walk that recursion with the same exactly rounded operations (slice_prop), the decide kernel consumes candidates in order,
// so the chain is the sequential one for every W, bit for bit.
#pragma once
#include "gpobj_kernels.h"
#include "parity_rng.h"

struct SliceChainState {
  int phase;            // 0: the evaluation at hyp_start is pending, 1: running, 2: finished, 3: stopped with an error
  int err;              // SLICE_ERR_*
  int stall;            // a proposal that had to be consumed failed its first (unjittered) factorisation: the host runs a checked round
  int sweep, idd, dd;   // 0-based sweep, position in its permutation, the open coordinate
  int shrink;           // proposals of the open coordinate consumed so far
  int maxshrink, nrec, rounds;
  long long funccount;  // evaluations the sequential algorithm needs (the reference's funccount)
  long long performed;  // evaluations launched
  double log_Px, log_uprime, xl, xr, err_newval;
};
enum { SLICE_ERR_NONE = 0, SLICE_ERR_COLLAPSE = 1, SLICE_ERR_X0 = 2, SLICE_ERR_UNIFORMS = 3 };
#define SLICE_MAXW 16
#define SLICE_MAXHYP 128
static_assert(SLICE_MAXHYP >= (VBMC_LIM_D + 1) + 4 + (2 * VBMC_LIM_D + 1), "k_slice_decide keeps Nhyp doubles in LDS arrays of SLICE_MAXHYP");

struct SliceKernelArgs : GpObjArgs {           // (hyp, sn2, scal, lp: one row per speculative candidate, W of them)
  int D, W, Kmax, Ns, thin, burn, adaptive, total, parity, has_base;
  unsigned long long seed;
  const double *LB, *UB, *LBo, *UBo;          // Nhyp: bounds, LB - eps(LB), UB + eps(UB)
  const double* basew;                        // Nhyp: the caller's widths (:166)
  const int* perms;                           // total x Nhyp, 0-based
  const double* U;                            // parity: total x Nhyp x (2 + Kmax)
  SliceChainState* st;
  double *xx, *widths, *xsum, *xsq;           // Nhyp each
  unsigned char *act, *on;                    // W: factorise / solve this candidate
  const double* out;                          // [nlZ W | failure index W] of k_nlz_final
  double *samples, *logp;                     // Ns x Nhyp (column-major), Ns
};

// The packed blocks of vbmc_gp_slice_sample, from the shape alone (nU: the parity uniforms, 0 without):
//   in:  X | y | s2 | LB UB LBo UBo | pmu psig pdf pc | basew | xx widths xsum xsq | U      ints: perms | ptype
//   flags: act | on (SLICE_MAXW each)                                                        smp: samples | logp
struct SliceBlocks {
  DevLayout in, ints, flags, smp;
  GpObjHead head;
  GpObjPrior prior;
  DevWin<double> LB, UB, LBo, UBo, basew, xx, widths, xsum, xsq, U, samples, logp;
  DevWin<int> perms, ptype;
  DevWin<unsigned char> act, on;
  SliceBlocks(int N, int D, int Nhyp, bool has_s2, size_t total, size_t nU, int Ns) {
    head.add(in, N, D, has_s2);
    LB = in.add<double>(Nhyp); UB = in.add<double>(Nhyp); LBo = in.add<double>(Nhyp); UBo = in.add<double>(Nhyp);
    prior.add(in, Nhyp);
    basew = in.add<double>(Nhyp); xx = in.add<double>(Nhyp); widths = in.add<double>(Nhyp); xsum = in.add<double>(Nhyp); xsq = in.add<double>(Nhyp);
    U = in.add_if<double>(nU != 0, nU);
    perms = ints.add<int>(total * Nhyp); ptype = ints.add<int>(Nhyp);
    act = flags.add<unsigned char>(SLICE_MAXW); on = flags.add<unsigned char>(SLICE_MAXW);
    samples = smp.add<double>((size_t)Ns * Nhyp); logp = smp.add<double>(Ns);
  }
  double* bind(SliceKernelArgs& a, void* din, void* dints, void* dflags, void* dsmp) const {   // returns X
    prior.bind(a, din);
    a.LB = LB.at(din); a.UB = UB.at(din); a.LBo = LBo.at(din); a.UBo = UBo.at(din); a.basew = basew.at(din);
    a.xx = xx.at(din); a.widths = widths.at(din); a.xsum = xsum.at(din); a.xsq = xsq.at(din); a.U = U.at(din);
    a.perms = perms.at(dints); a.ptype = ptype.at(dints);
    a.act = act.at(dflags); a.on = on.at(dflags);
    a.samples = samples.at(dsmp); a.logp = logp.at(dsmp);
    return head.bind(a, din);
  }
};

// slot 0: slice level (:245), 1: interval placement (:252), 2 + k: k-th shrink proposal (:286).  NaN: the parity block has no such slot.
__device__ __forceinline__ double slice_u(const SliceKernelArgs& a, int sweep, int idd, int slot) {
  if (!a.parity) return slice_uniform(a.seed, (unsigned)sweep, (unsigned)idd, (unsigned)slot);
  if (slot >= 2 + a.Kmax) return __builtin_nan("");
  return a.U[((size_t)sweep * a.Nhyp + idd) * (size_t)(2 + a.Kmax) + slot];
}

// One workgroup per candidate w: the candidate's hyper-parameter vector, its noise vector / Cholesky branch (gplite_core.m:33-40,67,
// gplite_noisefun.m:176-210) and its hyper-prior (gplite_hypprior.m:17-65).  checked != 0: the host's answer to a stall.
__global__ void __launch_bounds__(256) k_slice_propose(SliceKernelArgs a, int checked) {
#pragma clang fp contract(off)
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SliceChainState* st = a.st;
  const int phase = st->phase;
  const bool live = phase <= 1 && (!st->stall || checked);
  bool active = live;
  const int dd = phase == 1 ? st->dd : -1;
  double xp = 0.0;
  if (live && phase == 0) active = w == 0;
  if (live && phase == 1) {
    double xl = st->xl, xr = st->xr;
    const double x0 = a.xx[dd];
    const int sweep = st->sweep, idd = st->idd, k0 = st->shrink;
    for (int j = 0; j <= w; ++j) {
      const double u = slice_u(a, sweep, idd, 2 + k0 + j);
      if (u != u) { active = false; break; }
      xp = slice_prop(u, xl, xr);
      if (j == w) break;
      if (xp > x0) xr = xp;
      else if (xp < x0) xl = xp;
      else { active = false; break; }          // the interval collapsed before this candidate: it is never reached
    }
    if (xp < a.LB[dd] || xp > a.UB[dd]) active = false;   // logpdfbound (:421): -Inf without an evaluation
  }
  if (tid == 0) { a.act[w] = active; a.on[w] = active; }
  if (!active) return;                                    // (workgroup-uniform)
  gpobj_emit<false>(a, w, [&](int i) { return i == dd ? xp : a.xx[i]; });
}

// One wave.  Lane j judges candidate j; the first terminal event in candidate order (accept, exhausted uniforms, a failed first try,
// a rejected proposal AT the current point) is found by ballot.  Everything after it is wave-uniform bookkeeping, lanes along Nhyp.
__global__ void __launch_bounds__(64) k_slice_decide(SliceKernelArgs a, int checked) {
#pragma clang fp contract(off)
  SliceChainState* st = a.st;
  const int lane = threadIdx.x, W = a.W, Nhyp = a.Nhyp;
  int phase = st->phase;
  if (phase >= 2) return;
  const bool was_stalled = st->stall != 0;
  if (was_stalled && !checked) return;
  __shared__ double xx[SLICE_MAXHYP], wd[SLICE_MAXHYP];
  for (int i = lane; i < Nhyp; i += 64) { xx[i] = a.xx[i]; wd[i] = a.widths[i]; }
  __syncthreads();
  int sweep = st->sweep, idd = st->idd, dd = st->dd, shrink = st->shrink, maxshrink = st->maxshrink, nrec = st->nrec, err = 0, stall = 0;
  long long funccount = st->funccount, performed = st->performed;
  double log_Px = st->log_Px, log_uprime = st->log_uprime, xl = st->xl, xr = st->xr, err_newval = 0.0;
  const double ninf = -__builtin_inf();
  // the value of candidate `lane`: -(nlZ - lp)  (gplite_train.m:528-538), NaN -> -Inf (slicesamplebnd.m:442)
  const bool mine = lane < W;
  const bool launched = mine && a.act != nullptr && a.on[lane];
  const bool pfail = launched && a.out[W + lane] > 0.0;
  double val = ninf;
  if (launched && !pfail) { val = -(a.out[lane] - a.lp[lane]); if (val != val) val = ninf; }
  performed += __popcll(__ballot(launched));
  bool accepted = false;
  if (phase == 0) {
    if (pfail && lane == 0 && !checked) stall = 1;
    stall = __shfl(stall, 0, 64);
    if (!stall) {
      const double v0 = __shfl(val, 0, 64);
      funccount = 1;
      if (!(v0 > ninf && v0 < __builtin_inf())) { phase = 3; err = SLICE_ERR_X0; err_newval = v0; }
      else { log_Px = v0; phase = 1; sweep = 0; idd = -1; accepted = true; }
    }
  } else {
    const double x0 = xx[dd];
    const double u = mine ? slice_u(a, sweep, idd, 2 + shrink + lane) : 0.0;
    // the recursion of the shrink loop, candidate by candidate (wave-uniform; lane j keeps what belongs to candidate j)
    double cxl = xl, cxr = xr, my_xp = 0.0, my_xl = xl, my_xr = xr;
    bool dead = false, my_dead = true, my_exh = false, my_at = false;
    for (int j = 0; j < W; ++j) {
      const double uj = __shfl(u, j, 64);
      const bool exh = uj != uj;
      const double xp = slice_prop(uj, cxl, cxr);
      const bool at = !(xp > x0) && !(xp < x0);
      if (!exh && !dead) {
        if (xp > x0) cxr = xp;
        else if (xp < x0) cxl = xp;
      }
      if (lane == j) { my_xp = xp; my_dead = dead; my_exh = exh && !dead; my_at = at && !exh && !dead; my_xl = cxl; my_xr = cxr; }
      if (exh || at) dead = true;
    }
    const bool inb = mine && !my_dead && !my_exh && !(my_xp < a.LB[dd] || my_xp > a.UB[dd]);
    const bool t_fail = inb && pfail && !checked;
    const bool t_acc = inb && !t_fail && val > log_uprime;
    const bool t_col = mine && !my_dead && my_at && !t_acc && !t_fail;
    const unsigned long long m_evt = __ballot(t_acc || t_fail || t_col || (mine && my_exh));
    const int f = m_evt ? __ffsll((long long)m_evt) - 1 : W - 1;    // the last candidate consumed
    const unsigned long long upto = f >= 63 ? ~0ull : ((1ull << (f + 1)) - 1ull);
    const int f_exh = __shfl((int)my_exh, f, 64), f_fail = __shfl((int)t_fail, f, 64), f_acc = __shfl((int)t_acc, f, 64), f_col = __shfl((int)t_col, f, 64);
    const double f_xp = __shfl(my_xp, f, 64), f_val = __shfl(val, f, 64), f_xl = __shfl(my_xl, f, 64), f_xr = __shfl(my_xr, f, 64);
    const int counted = __popcll(__ballot(inb) & upto);             // funccount (:440): evaluations inside the bounds, NaN included
    if (m_evt && f_fail) stall = 1;
    else if (m_evt && f_exh) {
      // (the candidates before f were rejected: they count)
      funccount += __popcll(__ballot(inb) & (upto >> 1));
      phase = 3; err = SLICE_ERR_UNIFORMS;
    } else {
      funccount += counted;
      shrink += f + 1;
      if (m_evt && f_acc) {
        log_Px = f_val;
        accepted = true;
        if (shrink > maxshrink) maxshrink = shrink;
        // width adaptation during burn-in (:307-318)
        if (sweep + 1 <= a.burn && a.adaptive && lane == 0) {
          const double delta = a.UB[dd] - a.LB[dd];
          const bool fin = delta > ninf && delta < __builtin_inf();
          if (shrink > 3) wd[dd] = fmax(wd[dd] / 1.1, fin ? matlab_eps(delta) : 2.220446049250313e-16);
          else if (shrink < 2) wd[dd] = fmin(wd[dd] * 1.2, delta);
        }
        if (lane == 0) xx[dd] = f_xp;                                // (:325)
        __syncthreads();
      } else if (m_evt && f_col) {
        phase = 3; err = SLICE_ERR_COLLAPSE; err_newval = f_val;     // (:298-301)
      } else { xl = f_xl; xr = f_xr; }                               // all W rejected: the coordinate stays open
    }
  }
  // next coordinate; the bookkeeping of a finished sweep on the way (:328-358)
  while (accepted) {
    ++idd;
    if (idd == Nhyp) {
      const int ii = sweep + 1;
      if (ii > a.burn && (ii - a.burn - 1) % a.thin == 0) {
        const int is = (ii - a.burn - 1) / a.thin;
        for (int i = lane; i < Nhyp; i += 64) a.samples[(size_t)is + (size_t)a.Ns * i] = xx[i];
        if (lane == 0) a.logp[is] = log_Px;
        ++nrec;
      }
      if (ii <= a.burn && 2 * ii > a.burn) {
        for (int i = lane; i < Nhyp; i += 64) {
          a.xsum[i] = a.xsum[i] + xx[i];
          a.xsq[i] = a.xsq[i] + xx[i] * xx[i];
        }
        if (ii == a.burn && a.adaptive) {
          const double bs = (double)(a.burn / 2);
          double nw[SLICE_MAXHYP / 64];
          bool neg = false;
#pragma unroll
          for (int q = 0; q < SLICE_MAXHYP / 64; ++q) {
            const int i = lane + 64 * q;
            nw[q] = 0.0;
            if (i < Nhyp) {
              const double m = a.xsum[i] / bs;
              const double v = a.xsq[i] / bs - m * m;
              neg |= v < 0.0;                                        // ~isreal(newwidths) (:349)
              nw[q] = fmin(5.0 * __dsqrt_rn(v), a.UBo[i] - a.LBo[i]);
            }
          }
          const bool anyneg = __ballot(neg) != 0ull;
#pragma unroll
          for (int q = 0; q < SLICE_MAXHYP / 64; ++q) {
            const int i = lane + 64 * q;
            if (i < Nhyp) {
              const double t = anyneg ? wd[i] : nw[q];
              wd[i] = a.has_base ? fmax(t, __dsqrt_rn(t * a.basew[i])) : t;
            }
          }
        }
      }
      __syncthreads();
      ++sweep;
      idd = 0;
      if (sweep == a.total) { phase = 2; break; }
    }
    dd = a.perms[(size_t)sweep * Nhyp + idd];
    const double lb = a.LB[dd], ub = a.UB[dd];
    if (lb == ub) continue;                                          // fixed dimension (:243)
    const double u0 = slice_u(a, sweep, idd, 0), rr = slice_u(a, sweep, idd, 1);
    log_uprime = log(u0) + log_Px;                         // (:245)
    xl = xx[dd] - rr * wd[dd];                   // (:253-254)
    xr = xx[dd] + (1.0 - rr) * wd[dd];
    if ((lb > ninf && lb < __builtin_inf()) || (ub > ninf && ub < __builtin_inf())) {
      xl = fmax(xl, a.LBo[dd]);                                      // (:257-260; MATLAB's max / min pass over a NaN bound)
      xr = fmin(xr, a.UBo[dd]);
    }
    shrink = 0;
    break;
  }
  __syncthreads();
  for (int i = lane; i < Nhyp; i += 64) { a.xx[i] = xx[i]; a.widths[i] = wd[i]; }
  if (lane == 0) {
    st->phase = phase; st->err = err; st->stall = stall;
    st->sweep = sweep; st->idd = idd; st->dd = dd; st->shrink = shrink; st->maxshrink = maxshrink; st->nrec = nrec;
    st->rounds = st->rounds + 1;
    st->funccount = funccount; st->performed = performed;
    st->log_Px = log_Px; st->log_uprime = log_uprime; st->xl = xl; st->xr = xr;
    if (err) st->err_newval = err_newval;
  }
}

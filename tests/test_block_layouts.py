"""CPU check of the named layouts of the packed device blocks (vbmc_amd/csrc: one struct per block beside the kernel arguments it serves,
built on dev_layout.h).  A stand-alone program that includes the headers holding them -- no HIP call, the host side built with the
address and undefined-behaviour sanitizers -- prints, for a shape given on its command line, every block's size and every window's byte
offset (-1: the window is absent, its pointer null).  The expected figures are the hand-written size formulas and running pointers of
commit b446fb6, the last one that carved the blocks by hand, transcribed below as arithmetic with the file and line each comes from.

The shapes are the smallest at which a layout can go wrong: everything 1 (N = 2), every count different and greater than 1 (Nm = 5, so
that the closing prediction's tile rounding Nap = 16 differs from it; S = 3, so that the flag bytes do not fill a double), and every
optional window present and absent: s2, the parity tails U / Z / B, hist_cap and trace_cap 0 and > 0, a posterior with and without a
trinfo, Step 2 off (W = 0, where x0 keeps max(W, 1) walkers), the gradient of gplite_nlZ, the noise estimate of the surrogate sampler."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include "gp_factor.h"
#include "slice_kernels.h"
#include "trainopt_kernels.h"
#include "search_kernels.h"
#include "is_setup_kernels.h"
#include "imiqr_target.h"
#include "gp_surrogate_kernels.h"
#include "mode_kernels.h"
#include "mtv_kernels.h"

static std::map<std::string, long long> arg;
static long long A(const char* k) { if (!arg.count(k)) { std::printf("missing %s\n", k); std::exit(2); } return arg[k]; }
static void size(const char* name, size_t bytes) { std::printf("%s %zu\n", name, bytes); }
template <class T> static void win(const char* name, const DevWin<T>& w) {
  char probe[1];
  std::printf("%s %lld\n", name, w.at((void*)probe) ? (long long)w.off : -1ll);
}
// every window's last element of a heap image of exactly bytes() bytes is written: the sanitizer sees a layout that overruns its size
template <class T> static void touch(const DevLayout& L, const DevWin<T>& w) {
  if (!w.n || !w.present) return;
  char* img = (char*)std::malloc(L.bytes());
  const T v{};
  std::memcpy((char*)w.at(img) + (w.n - 1) * sizeof(T), &v, sizeof(T));
  std::free(img);
}
#define W(L, name, w) do { win(name, w); touch(L, w); } while (0)

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) { std::string s(argv[i]); const size_t e = s.find('='); arg[s.substr(0, e)] = std::atoll(s.c_str() + e + 1); }
  const int N = A("N"), D = A("D"), Nhyp = A("Nhyp"), S = A("S"), K = A("K"), Wd = A("W"), lam = A("lam"), Nm = A("Nm"), E = A("E"), C = A("C");
  const bool s2 = A("s2"), parity = A("parity"), trinfo = A("trinfo"), grad = A("grad");
  std::printf("VPT_MAXBLK %d\nSLICE_MAXW %d\nIS_SLOTS %d\n", VPT_MAXBLK, SLICE_MAXW, IS_SLOTS);
  {
    const size_t total = A("total"), nU = parity ? total * Nhyp * (2 + A("Kmax")) : 0;
    const SliceBlocks L(N, D, Nhyp, s2, total, nU, A("Ns"));
    size("slice.in", L.in.bytes()); size("slice.ints", L.ints.bytes()); size("slice.flags", L.flags.bytes()); size("slice.smp", L.smp.bytes());
    W(L.in, "slice.X", L.head.X); W(L.in, "slice.y", L.head.y); W(L.in, "slice.s2", L.head.s2);
    W(L.in, "slice.LB", L.LB); W(L.in, "slice.UB", L.UB); W(L.in, "slice.LBo", L.LBo); W(L.in, "slice.UBo", L.UBo);
    W(L.in, "slice.pmu", L.prior.pmu); W(L.in, "slice.psig", L.prior.psig); W(L.in, "slice.pdf", L.prior.pdf); W(L.in, "slice.pc", L.prior.pc);
    W(L.in, "slice.basew", L.basew); W(L.in, "slice.xx", L.xx); W(L.in, "slice.widths", L.widths); W(L.in, "slice.xsum", L.xsum); W(L.in, "slice.xsq", L.xsq);
    W(L.in, "slice.U", L.U);
    W(L.ints, "slice.perms", L.perms); W(L.ints, "slice.ptype", L.ptype); W(L.flags, "slice.act", L.act); W(L.flags, "slice.on", L.on);
    W(L.smp, "slice.samples", L.samples); W(L.smp, "slice.logp", L.logp);
  }
  {
    const ToptBlocks L(N, D, Nhyp, s2, A("Nrows"), A("Nopts"), A("BB"), A("hist_cap"));
    size("topt.in", L.in.bytes()); size("topt.ints", L.ints.bytes()); size("topt.vec", L.vec.bytes()); size("topt.lp", L.lp.bytes());
    size("topt.flags", L.flags.bytes()); size("topt.fill", L.fill.bytes()); size("topt.res", L.res.bytes()); size("topt.hist", L.hist.bytes());
    W(L.in, "topt.X", L.head.X); W(L.in, "topt.y", L.head.y); W(L.in, "topt.s2", L.head.s2); W(L.in, "topt.LB", L.LB); W(L.in, "topt.UB", L.UB);
    W(L.in, "topt.pmu", L.prior.pmu); W(L.in, "topt.psig", L.prior.psig); W(L.in, "topt.pdf", L.prior.pdf); W(L.in, "topt.pc", L.prior.pc);
    W(L.in, "topt.design", L.design);
    W(L.ints, "topt.ptype", L.ptype); W(L.ints, "topt.order", L.order); W(L.ints, "topt.best", L.best); W(L.ints, "topt.hist_k", L.hist_k);
    W(L.vec, "topt.x", L.x); W(L.vec, "topt.g", L.g); W(L.vec, "topt.d", L.d); W(L.lp, "topt.lp.lp", L.lpv); W(L.lp, "topt.dlp", L.dlp);
    W(L.flags, "topt.act", L.act); W(L.flags, "topt.on", L.on);
    W(L.fill, "topt.fvals", L.fvals); W(L.fill, "topt.fsorted", L.fsorted); W(L.fill, "topt.widths", L.widths);
    W(L.res, "topt.res_nll", L.res_nll); W(L.res, "topt.hyp_start", L.hyp_start); W(L.hist, "topt.hist_f", L.hist_f); W(L.hist, "topt.hist_x", L.hist_x);
  }
  {
    const int mu = lam / 2, nh = A("nh");
    const SearchBlocks L(D, lam, mu, nh, parity ? (size_t)D * lam * A("Gmax") : 0, A("tcap"));
    size("search.w", L.w.bytes()); size("search.fixed", L.fixed); size("search.trd", L.trd.bytes());
    W(L.w, "search.wts", L.wts); W(L.w, "search.LB", L.LB); W(L.w, "search.UB", L.UB); W(L.w, "search.xmean", L.xmean); W(L.w, "search.ps", L.ps);
    W(L.w, "search.pc", L.pc); W(L.w, "search.xbest", L.xbest); W(L.w, "search.xlast", L.xlast); W(L.w, "search.C", L.C); W(L.w, "search.A", L.A);
    W(L.w, "search.Y", L.Y); W(L.w, "search.hist", L.hist); W(L.w, "search.F", L.F); W(L.w, "search.fbar", L.fbar); W(L.w, "search.vtot", L.vtot);
    W(L.w, "search.Z", L.Z); W(L.trd, "search.tr_F", L.tr_F); W(L.trd, "search.tr_xmean", L.tr_xmean); W(L.trd, "search.tr_sigma", L.tr_sigma);
  }
  {
    const ImiqrExtra X(S, C, Nm);
    const IsCoreBlock L(D, S, Wd, C, Nm, X.L, parity ? (size_t)IS_SLOTS * (Wd / 2) * S * A("Mmax") : 0);
    size("is.w", L.w.bytes()); size("is.fixed", L.fixed); size("imiqr.extra", X.L.bytes());
    W(L.w, "is.LB", L.LB); W(L.w, "is.UB", L.UB); W(L.w, "is.x", L.x); W(L.w, "is.lp", L.lp); W(L.w, "is.P", L.P); W(L.w, "is.val", L.val);
    W(L.w, "is.extra", L.extra); W(L.w, "is.Xa", L.Xa); W(L.w, "is.rlp", L.rlp); W(L.w, "is.U", L.U);
    W(X.L, "imiqr.fmu", X.fmu); W(X.L, "imiqr.fs2", X.fs2); W(X.L, "imiqr.ys2", X.ys2); W(X.L, "imiqr.cl_logp", X.cl_logp); W(X.L, "imiqr.cl_fmu", X.cl_fmu);
    W(X.L, "imiqr.cl_fs2", X.cl_fs2); W(X.L, "imiqr.cl_ys2", X.cl_ys2); W(X.L, "imiqr.lnw", X.lnw); W(X.L, "imiqr.fs2a", X.fs2a);
  }
  {
    const GsBlocks G(D, S, E, C, (size_t)Wd * E * D, A("Nnn"));
    const IsCoreBlock L(D, E, Wd, C, Nm, G.extra, 0);
    size("gs.extra", G.extra.bytes()); size("gs.v", G.v.bytes()); size("gs.x0", G.x0.bytes()); size("gs.nn", G.nn.bytes()); size("gs.is.w", L.w.bytes());
    W(G.extra, "gs.ymu", G.ymu); W(G.extra, "gs.ys2", G.ys2); W(G.v, "gs.vt", G.vt); W(G.v, "gs.sum", G.sum); W(G.v, "gs.part", G.part);
    W(G.x0, "gs.start", G.start); W(G.x0, "gs.clipped", G.clipped); W(G.nn, "gs.draws", G.draws); W(G.nn, "gs.sn2", G.sn2);
    W(L.w, "gs.is.extra", L.extra); W(L.w, "gs.is.Xa", L.Xa);
  }
  {
    const int Wq = A("step2") ? Wd : 0;
    const IsSetupBlock L(D, S, K, Wq, A("Na1"), parity);
    size("setup", L.L.bytes()); size("setup.upload", L.upload); size("setup.block_len", IsSetupBlock::block_len(D, S, Wq, A("Na1")) * 8);
    W(L.L, "setup.mu", L.mu); W(L.L, "setup.sigma", L.sigma); W(L.L, "setup.lambda", L.lambda); W(L.L, "setup.w", L.w); W(L.L, "setup.B", L.B);
    W(L.L, "setup.geo", L.geo); W(L.L, "setup.comp", L.comp); W(L.L, "setup.Xa1", L.Xa1); W(L.L, "setup.P", L.P); W(L.L, "setup.logp", L.logp);
    W(L.L, "setup.fmu", L.fmu); W(L.L, "setup.fs2", L.fs2); W(L.L, "setup.ys2", L.ys2); W(L.L, "setup.lpdf", L.lpdf); W(L.L, "setup.lnw1", L.lnw1);
    W(L.L, "setup.fs2a1", L.fs2a1); W(L.L, "setup.lw", L.lw); W(L.L, "setup.x0", L.x0);
  }
  {
    const int DT = A("DT"), Kp = (K + 63) / 64 * 64, Sm = A("ranked") ? A("nmax") : K;
    const ModeBlocks L(D, DT, K, Kp, Sm);
    size("mode.b", L.b.bytes()); size("mode.res", L.res.bytes()); size("mode.i", L.i.bytes());
    W(L.b, "mode.muT", L.muT); W(L.b, "mode.f_all", L.f_all); W(L.b, "mode.results", L.results);
    W(L.res, "mode.f0", L.f0); W(L.res, "mode.fs", L.fs); W(L.res, "mode.us", L.us); W(L.res, "mode.xs", L.xs);
    W(L.i, "mode.start_comp", L.start_comp); W(L.i, "mode.iters", L.iters); W(L.i, "mode.nfev", L.nfev); W(L.i, "mode.stop", L.stop);
    const VptPackLayout P(D, DT, K, trinfo);
    size("vpt", P.L.bytes());
    W(P.L, "vpt.mus", P.mus); W(P.L, "vpt.cst", P.cst); W(P.L, "vpt.is2", P.is2); W(P.L, "vpt.mu", P.mu); W(P.L, "vpt.sig", P.sig); W(P.L, "vpt.lam", P.lam);
    W(P.L, "vpt.ilam", P.ilam); W(P.L, "vpt.tr", P.tr);
  }
  {
    const size_t xin = A("extra_in"), nG = (size_t)S * GPC_STRIDE(D);
    const GpPackLayout L(N, D, S, Nhyp, xin);
    size("gppack", L.L.bytes()); size("gppack.total", L.total * 8);
    W(L.L, "gppack.X", L.X); W(L.L, "gppack.y", L.y); W(L.L, "gppack.hyp", L.hyp); W(L.L, "gppack.sn2", L.sn2); W(L.L, "gppack.scal", L.scal);
    W(L.L, "gppack.ones", L.ones); W(L.L, "gppack.needinv", L.needinv); W(L.L, "gppack.active", L.active); W(L.L, "gppack.lchol", L.lchol);
    W(L.L, "gppack.extra", L.extra);
    const GpPostExtra X(D, S, nG);
    size("gppost", X.L.bytes());
    W(X.L, "gppost.gpc", X.gpc); W(X.L, "gppost.sn2_eff", X.sn2_eff); W(X.L, "gppost.meanX", X.meanX); W(X.L, "gppost.mult", X.mult);
    const GpNlzOut O(S, Nhyp, grad);
    size("nlzout", O.L.bytes());
    W(O.L, "nlzout.nlZ", O.nlZ); W(O.L, "nlzout.pfd", O.pfd); W(O.L, "nlzout.dnlZ", O.dnlZ);
    const GpRank1Block R(N + 1, D, S, Nhyp, nG);
    size("rank1", R.L.bytes()); size("rank1.upload", R.upload * 8);
    W(R.L, "rank1.X", R.X); W(R.L, "rank1.meanX", R.meanX); W(R.L, "rank1.hyp", R.hyp); W(R.L, "rank1.gpc", R.gpc); W(R.L, "rank1.sn2_eff", R.sn2_eff);
    W(R.L, "rank1.mult", R.mult); W(R.L, "rank1.lchol", R.lchol);
  }
  {
    const size_t nb = A("nb"), nent = A("nent"), nC = A("nC"), nmsh = A("nmsh"), ngeo = A("ngeo");
    const VptReduceBlock M(nb * nent, nent), Kl(2 * nb, 2);
    const VptMomEntries En((int)nent);
    size("mom.p", M.L.bytes()); size("mom.e", En.L.bytes()); size("kl.p", Kl.L.bytes());
    W(M.L, "mom.partial", M.partial); W(M.L, "mom.out", M.out); W(En.L, "mom.ei", En.ei); W(En.L, "mom.ej", En.ej);
    W(Kl.L, "kl.partial0", Kl.partial.part(0, nb)); W(Kl.L, "kl.partial1", Kl.partial.part(nb, nb)); W(Kl.L, "kl.out", Kl.out);
    const MtvWork Tw(nC);
    const MtvIntBlocks T(nC, nmsh, ngeo);
    size("mtv.w", Tw.w.bytes()); size("mtv.s", T.s.bytes()); size("mtv.g", T.g.bytes());
    W(Tw.w, "mtv.x", Tw.x); W(Tw.w, "mtv.a", Tw.a); W(Tw.w, "mtv.a2", Tw.a2); W(Tw.w, "mtv.at", Tw.at); W(Tw.w, "mtv.raw", Tw.raw);
    W(T.s, "mtv.yy", T.yy); W(T.s, "mtv.mm", T.mm); W(T.g, "mtv.msh", T.msh); W(T.g, "mtv.geo", T.geo);
  }
  return 0;
}
"""

BASE = dict(N=2, D=1, Nhyp=1, S=1, K=1, W=1, lam=1, Nm=1, E=1, C=1, total=1, Kmax=1, Ns=1, Nrows=1, Nopts=1, BB=1, hist_cap=0, tcap=0, Gmax=1, nh=40,
            Mmax=1, Nnn=0, Na1=1, step2=1, DT=4, ranked=0, nmax=1, extra_in=0, nb=1, nent=1, nC=1, nmsh=4, ngeo=4,
            s2=0, parity=0, trinfo=0, grad=0)
DISTINCT = dict(N=5, D=3, Nhyp=7, S=2, K=4, W=6, lam=6, Nm=5, E=3, C=18, total=9, Kmax=2, Ns=11, Nrows=13, Nopts=2, BB=13, hist_cap=0, tcap=0, Gmax=3,
                nh=25, Mmax=4, Nnn=0, Na1=17, step2=1, DT=4, ranked=0, nmax=3, extra_in=10, nb=3, nent=9, nC=24, nmsh=24, ngeo=36,
                s2=0, parity=0, trinfo=0, grad=0)
CASES = {
    "ones": BASE,
    "ones_all_present": dict(BASE, s2=1, parity=1, hist_cap=1, tcap=1, trinfo=1, grad=1, Nnn=1, ranked=1),
    "distinct_all_absent": DISTINCT,
    "distinct_all_present": dict(DISTINCT, s2=1, parity=1, hist_cap=5, tcap=4, trinfo=1, grad=1, Nnn=8, ranked=1),
    "s3_flags_not_a_double": dict(DISTINCT, S=3, s2=1, grad=1),
    "step2_off": dict(DISTINCT, step2=0, parity=1),
    "only_s2": dict(DISTINCT, s2=1),
    "only_parity": dict(DISTINCT, parity=1),
    "only_hist_and_trace": dict(DISTINCT, hist_cap=3, tcap=2),
    "only_trinfo_ranked": dict(DISTINCT, trinfo=1, ranked=1, DT=8),
}


def _chain(out, prefix, fields, unit=8, start=0):
    """windows back to back from `start` (in units): out[prefix.name] = byte offset; returns the end in units"""
    o = start
    for name, n in fields:
        out[prefix + name] = o * unit
        o += n
    return o


def expected(p, const):
    """the parent's sizes and offsets (b446fb6), in bytes; -1: a null pointer"""
    N, D, Nhyp, S, K, W, lam, Nm, E, C = (p[k] for k in ("N", "D", "Nhyp", "S", "K", "W", "lam", "Nm", "E", "C"))
    x = {}
    # ---- vbmc_gp_slice_sample
    total, Ns = p["total"], p["Ns"]
    nX = N * D
    nU = total * Nhyp * (2 + p["Kmax"]) if p["parity"] else 0                                  # abi_gp_train.hip:148
    x["slice.in"] = (nX + 2 * N + 13 * Nhyp + nU) * 8                                         # :152
    x["slice.ints"] = (total * Nhyp + Nhyp) * 4                                               # :156
    x["slice.flags"] = 2 * const["SLICE_MAXW"]                                                # :162
    x["slice.smp"] = (Ns * Nhyp + Ns) * 8                                                     # :165
    x["slice.X"], x["slice.y"] = 0, nX * 8                                                    # :197-198
    x["slice.s2"] = (nX + N) * 8 if p["s2"] else -1                                           # :199
    q = nX + 2 * N
    for i, name in enumerate(["LB", "UB", "LBo", "UBo", "pmu", "psig", "pdf", "pc", "basew", "xx", "widths", "xsum", "xsq"]):
        x["slice." + name] = (q + i * Nhyp) * 8                                               # :200-201
    x["slice.U"] = (q + 13 * Nhyp) * 8 if nU else -1                                          # :202
    x["slice.perms"], x["slice.ptype"] = 0, total * Nhyp * 4                                  # :203
    x["slice.act"], x["slice.on"] = 0, const["SLICE_MAXW"]                                    # :206
    x["slice.samples"], x["slice.logp"] = 0, Ns * Nhyp * 8                                    # :207
    # ---- vbmc_gp_train_optimize
    Nrows, Nopts, BB, hc = p["Nrows"], p["Nopts"], p["BB"], p["hist_cap"]
    x["topt.in"] = (nX + 2 * N + 6 * Nhyp + Nrows * Nhyp) * 8                                 # :309
    x["topt.ints"] = (Nhyp + Nrows + 1 + Nopts * hc + 1) * 4                                  # :314
    x["topt.vec"] = 3 * Nopts * Nhyp * 8                                                      # :316
    x["topt.lp"] = (BB + BB * Nhyp) * 8                                                       # :322
    x["topt.flags"] = 2 * BB                                                                  # :323
    x["topt.fill"] = (2 * Nrows + Nhyp) * 8                                                   # :330
    x["topt.res"] = (Nopts + Nhyp) * 8                                                        # :331
    x["topt.hist"] = max(1, Nopts * hc * (Nhyp + 1)) * 8                                      # :332
    x["topt.X"], x["topt.y"] = 0, nX * 8                                                      # :365-366
    x["topt.s2"] = (nX + N) * 8 if p["s2"] else -1                                            # :367
    for i, name in enumerate(["LB", "UB", "pmu", "psig", "pdf", "pc", "design"]):
        x["topt." + name] = (q + i * Nhyp) * 8                                                # :368
    _chain(x, "topt.", [("ptype", Nhyp), ("order", Nrows), ("best", 1), ("hist_k", 0)], unit=4)   # :369
    _chain(x, "topt.", [("x", Nopts * Nhyp), ("g", Nopts * Nhyp), ("d", 0)])                  # :371
    x["topt.lp.lp"], x["topt.dlp"] = 0, BB * 8                                                # :372
    x["topt.act"], x["topt.on"] = 0, BB                                                       # :373
    _chain(x, "topt.", [("fvals", Nrows), ("fsorted", Nrows), ("widths", 0)])                 # :374
    x["topt.res_nll"], x["topt.hyp_start"] = 0, Nopts * 8                                     # :375
    x["topt.hist_f"], x["topt.hist_x"] = (0, Nopts * hc * 8) if hc else (-1, -1)              # :376
    # ---- vbmc_acq_search
    mu, nh, tcap = lam // 2, p["nh"], p["tcap"]
    nZ = D * lam * p["Gmax"] if p["parity"] else 0                                            # abi_acq_search.hip:143
    n_fixed = mu + 7 * D + 2 * D * D + D * lam + nh + 3 * lam                                 # :144
    x["search.w"], x["search.fixed"] = (n_fixed + nZ) * 8, n_fixed * 8                        # :147, :176
    x["search.trd"] = tcap * (lam + D + 1) * 8                                                # :151 (not allocated with tcap = 0)
    end = _chain(x, "search.", [("wts", mu), ("LB", D), ("UB", D), ("xmean", D), ("ps", D), ("pc", D), ("xbest", D), ("xlast", D), ("C", D * D), ("A", D * D),
                                ("Y", D * lam), ("hist", nh), ("F", lam), ("fbar", lam), ("vtot", lam)])   # :160-173
    assert end == n_fixed
    x["search.Z"] = n_fixed * 8 if nZ else -1                                                 # :174
    if tcap:
        _chain(x, "search.", [("tr_F", tcap * lam), ("tr_xmean", tcap * D), ("tr_sigma", 0)])   # :187
    else:
        x["search.tr_F"] = x["search.tr_xmean"] = x["search.tr_sigma"] = -1                   # :185
    # ---- the ensemble sampler with the IMIQR target (E = S) and with the surrogate's
    Nap = (Nm + 15) // 16 * 16                                                                # imiqr_target.h:30
    nv, nr, np_ = S * C, S * Nm, S * Nap                                                      # :29, :31
    extra = 3 * nv + 4 * nr + 2 * np_                                                         # :32
    x["imiqr.extra"] = extra * 8
    _chain(x, "imiqr.", [("fmu", nv), ("fs2", nv), ("ys2", nv), ("cl_logp", nr), ("cl_fmu", nr), ("cl_fs2", nr), ("cl_ys2", nr), ("lnw", np_), ("fs2a", np_)])   # :36-39, :59
    H = W // 2
    nUi = const["IS_SLOTS"] * H * S * p["Mmax"] if p["parity"] else 0                         # is_core.h:121
    nx, nP, nXa = S * W * D, S * D * C, Nm * D * S                                            # :122
    fixed = 2 * D + nx + S * W + nP + nv + extra + nXa + nr                                   # :123
    x["is.w"], x["is.fixed"] = (fixed + nUi) * 8, fixed * 8                                   # :125, :130
    end = _chain(x, "is.", [("LB", D), ("UB", D), ("x", nx), ("lp", S * W), ("P", nP), ("val", nv), ("extra", extra), ("Xa", nXa), ("rlp", nr)])   # :134-144
    assert end == fixed
    x["is.U"] = fixed * 8 if nUi else -1                                                      # :145
    nsv = S * E * C                                                                           # abi_gp_surrogate.hip:89
    x["gs.extra"] = 2 * nsv * 8                                                               # :90
    x["gs.ymu"], x["gs.ys2"] = 0, nsv * 8                                                     # :91
    x["gs.v"] = (3 + const["VPT_MAXBLK"]) * 8                                                 # :85
    x["gs.vt"], x["gs.sum"], x["gs.part"] = 0, 2 * 8, 3 * 8                                   # :132-134
    n0 = W * E * D                                                                            # :75
    x["gs.x0"], x["gs.start"], x["gs.clipped"] = 2 * n0 * 8, 0, n0 * 8                        # :108-109
    Nnn = p["Nnn"]
    x["gs.nn"], x["gs.draws"], x["gs.sn2"] = (Nnn * D + Nnn) * 8, 0, Nnn * D * 8              # :126-128
    gfixed = 2 * D + E * W * D + E * W + E * D * C + E * C + 2 * nsv + Nm * D * E + E * Nm    # is_core.h:123 with E ensembles
    x["gs.is.w"] = gfixed * 8
    x["gs.is.extra"] = (2 * D + E * W * D + E * W + E * D * C + E * C) * 8                    # :142
    x["gs.is.Xa"] = x["gs.is.extra"] + 2 * nsv * 8                                            # :143
    # ---- vbmc_acq_is_setup
    Wq = W if p["step2"] else 0                                                               # abi_is_setup.hip:54
    Na1 = p["Na1"]
    Nap1, K4 = (Na1 + 15) // 16 * 16, 4 * K                                                   # :45
    block_len = (D + 1) * Na1 + Wq * S                                                        # :12
    nB = block_len if p["parity"] else 0                                                      # :65
    nvp, nX1, nP1, nv1, np1 = D * K + K + D + K, Na1 * D, S * D * Na1, S * Na1, S * Nap1      # :83
    nx0 = max(Wq, 1) * D * S                                                                  # :84
    n1 = nvp + nB + (D + 1) + 3 * K4 + nX1 + nP1 + 4 * nv1 + Na1 + 2 * np1 + nv1 + nx0        # :85
    x["setup"], x["setup.upload"], x["setup.block_len"] = n1 * 8, (nvp + nB) * 8, block_len * 8   # :87, :90
    end = _chain(x, "setup.", [("mu", D * K), ("sigma", K), ("lambda", D), ("w", K), ("B", nB), ("geo", D + 1), ("comp", 3 * K4), ("Xa1", nX1), ("P", nP1),
                               ("logp", nv1), ("fmu", nv1), ("fs2", nv1), ("ys2", nv1), ("lpdf", Na1), ("lnw1", np1), ("fs2a1", np1), ("lw", nv1), ("x0", nx0)])   # :104-120, :127
    assert end == n1
    if not nB:
        x["setup.B"] = -1                                                                     # :109
    # ---- vbmc_vp_mode and the packed posterior
    DT, Kp = p["DT"], (K + 63) // 64 * 64                                                     # mode_host.h:17
    Sm = p["nmax"] if p["ranked"] else K                                                      # :13
    x["mode.b"] = (DT * Kp + K + 2 * Sm + 2 * Sm * D) * 8                                     # :22
    x["mode.res"] = (2 * Sm + 2 * Sm * D) * 8                                                 # :43
    x["mode.i"] = 4 * Sm * 4                                                                  # :25
    x["mode.muT"], x["mode.f_all"], x["mode.results"] = 0, DT * Kp * 8, (DT * Kp + K) * 8     # :29, :32-33
    _chain(x, "mode.", [("f0", Sm), ("fs", Sm), ("us", Sm * D), ("xs", 0)])                   # :33, :48
    _chain(x, "mode.", [("start_comp", Sm), ("iters", Sm), ("nfev", Sm), ("stop", 0)], unit=4)   # :34
    ntr = const["VPT_NROWS"] * DT + DT * DT if p["trinfo"] else 0                             # vp_tools_host.h:122
    end = _chain(x, "vpt.", [("mus", K * DT), ("cst", K), ("is2", K), ("mu", D * K), ("sig", K), ("lam", DT), ("ilam", DT), ("tr", ntr)])   # :114-122
    x["vpt"] = end * 8                                                                        # :123
    if not p["trinfo"]:
        x["vpt.tr"] = -1                                                                      # :163
    # ---- the GP entry points
    xin = p["extra_in"]
    y_ = N * D; hyp_ = y_ + N; sn2_ = hyp_ + Nhyp * S; scal_ = sn2_ + S * N; flags_ = scal_ + S * 4    # gp_factor.h:210
    extra_ = flags_ + (4 * S + 7) // 8; total_ = extra_ + xin                                 # :211
    x["gppack"] = x["gppack.total"] = total_ * 8                                              # :304
    x.update({"gppack.X": 0, "gppack.y": y_ * 8, "gppack.hyp": hyp_ * 8, "gppack.sn2": sn2_ * 8, "gppack.scal": scal_ * 8, "gppack.extra": extra_ * 8})
    for k, name in enumerate(["ones", "needinv", "active", "lchol"]):
        x["gppack." + name] = flags_ * 8 + k * S                                              # :213, :301-302
    nG = S * (3 * D + 2)                                                                      # elbo_types.h:27, abi_gp.hip:70
    x["gppost"] = (nG + S + D + S) * 8                                                        # abi_gp.hip:73
    _chain(x, "gppost.", [("gpc", nG), ("sn2_eff", S), ("meanX", D), ("mult", 0)])            # :154
    x["nlzout"] = S * (2 + (Nhyp if p["grad"] else 0)) * 8                                    # :217
    x["nlzout.nlZ"], x["nlzout.pfd"], x["nlzout.dnlZ"] = 0, S * 8, (2 * S * 8 if p["grad"] else -1)   # :245, :248-249
    N1 = N + 1
    nXn, nH = N1 * D, Nhyp * S                                                                # :448
    x["rank1"] = (nXn + D + nH + nG + 2 * S + (S + 7) // 8) * 8                               # :449
    x["rank1.upload"] = (nXn + D) * 8                                                         # :470
    _chain(x, "rank1.", [("X", nXn), ("meanX", D), ("hyp", nH), ("gpc", nG), ("sn2_eff", S), ("mult", S), ("lchol", 0)])   # :466-467
    # ---- moments, kldiv, the KDE pipeline
    nb, nent, nC, nmsh, ngeo = p["nb"], p["nent"], p["nC"], p["nmsh"], p["ngeo"]
    x["mom.p"], x["mom.partial"], x["mom.out"] = (nb + 1) * nent * 8, 0, nb * nent * 8        # abi_vp_tools.hip:130, :135-136
    x["mom.e"], x["mom.ei"], x["mom.ej"] = 2 * nent, 0, nent                                  # :117, :134
    x["kl.p"], x["kl.partial0"], x["kl.partial1"], x["kl.out"] = (2 * nb + 2) * 8, 0, nb * 8, 2 * nb * 8   # :183, :189, :193
    x["mtv.w"] = 5 * nC * 8                                                                   # mtv_host.h:137
    _chain(x, "mtv.", [("x", nC), ("a", nC), ("a2", nC), ("at", nC), ("raw", 0)])             # :178
    x["mtv.s"], x["mtv.yy"], x["mtv.mm"] = 2 * nC * 8, 0, nC * 8                              # :249, :253-254
    x["mtv.g"], x["mtv.msh"], x["mtv.geo"] = (nmsh + ngeo) * 8, 0, nmsh * 8                   # :250, :255-256
    return x


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("block_layouts"))
    src, exe = os.path.join(d, "block_layouts.hip"), os.path.join(d, "block_layouts")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("case", sorted(CASES))
def test_layouts_match_the_hand_carved_blocks(program, case):
    p = CASES[case]
    r = subprocess.run([program] + ["%s=%d" % kv for kv in sorted(p.items())], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = {}
    for line in r.stdout.splitlines():
        name, value = line.split()
        got[name] = int(value)
    const = {k: got.pop(k) for k in ("VPT_MAXBLK", "SLICE_MAXW", "IS_SLOTS")}
    const["VPT_NROWS"] = 8                                                                    # vp_tools_kernels.h:28
    want = expected(p, const)
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_the_table_reaches_every_optional_window_both_ways():
    for flag in ("s2", "parity", "trinfo", "grad", "ranked", "step2"):
        assert {CASES[c][flag] for c in CASES} == {0, 1}, flag
    for cap in ("hist_cap", "tcap", "Nnn"):
        assert {CASES[c][cap] > 0 for c in CASES} == {False, True}, cap
    d = CASES["distinct_all_absent"]
    assert (d["Nm"] + 15) // 16 * 16 != d["Nm"] and (4 * CASES["s3_flags_not_a_double"]["S"]) % 8 != 0
    assert math.prod(CASES["ones"][k] for k in ("D", "Nhyp", "S", "K", "W")) == 1 and CASES["ones"]["N"] == 2

"""Small GP training problems shared by the CPU and the GPU tests of the optimisation half of gplite_train."""
import numpy as np


def gp_case(seed, D=2, N=30, meanfun=4, noisefun=(1, 0, 0), prior="flat", fixed=None, infbound=None):
    """A dict: gp (the struct gplite_nlZ reads), h0, LB, UB, PLB, PUB, hprior (None for a flat prior).  The prior lies on the covariance
    hyper-parameters alone; "gauss-all", "student-all" and "mixed-all" put one on every coordinate (mixed: Gaussian on the even ones)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * (1.0 + 0.5 * np.arange(D))
    y = -0.5 * np.sum((X / (1.0 + np.arange(D))) ** 2, axis=1) + 0.3 * np.sin(X[:, 0]) + 0.05 * rng.standard_normal(N)
    nf = tuple(int(v) for v in noisefun)
    s2 = 0.01 + 0.02 * rng.random(N) if nf[1] else None
    hn, ln, un = [np.log(0.1)], [np.log(1e-3)], [np.log(3.0)]
    if nf[1] == 2:
        hn += [0.0]; ln += [-3.0]; un += [3.0]
    if nf[2] == 1:
        hn += [float(np.median(y)), np.log(0.1)]; ln += [float(np.min(y)) - 1.0, np.log(1e-3)]; un += [float(np.max(y)) + 1.0, np.log(3.0)]
    sx, sy = np.log(np.std(X, axis=0)), np.log(np.std(y))
    hm, lm, um = [], [], []
    if meanfun == 1:
        hm, lm, um = [float(np.mean(y))], [float(np.min(y)) - 5.0], [float(np.max(y)) + 5.0]
    elif meanfun == 4:
        hm = [float(np.max(y))] + list(np.mean(X, axis=0)) + list(sx)
        lm = [float(np.max(y)) - 10.0] + list(np.min(X, axis=0)) + list(sx - 3.0)
        um = [float(np.max(y)) + 10.0] + list(np.max(X, axis=0)) + list(sx + 3.0)
    h0 = np.array(list(sx) + [sy] + hn + hm, dtype=np.float64)
    LB = np.array(list(sx - 4.0) + [sy - 5.0] + ln + lm, dtype=np.float64)
    UB = np.array(list(sx + 4.0) + [sy + 5.0] + un + um, dtype=np.float64)
    PLB, PUB = h0 - 0.25 * (h0 - LB), h0 + 0.25 * (UB - h0)
    span = UB - LB                                     # (before a coordinate is fixed or freed: the scale of an "-all" prior)
    if fixed is not None:
        LB[fixed] = UB[fixed] = PLB[fixed] = PUB[fixed] = h0[fixed]
    if infbound is not None:
        LB[infbound], UB[infbound] = -np.inf, np.inf
    Nhyp = h0.size
    hprior = None
    prior, everywhere = (prior[:-4], True) if prior.endswith("-all") else (prior, False)
    if prior != "flat":
        mu, sg, df = np.full(Nhyp, np.nan), np.full(Nhyp, np.nan), np.full(Nhyp, np.nan)
        mu[:D + 1], sg[:D + 1] = h0[:D + 1] + 0.2, 1.5
        df[:D + 1] = 0.0 if prior == "gauss" else 3.0
        if prior == "mixed":
            df[0] = 0.0
        if everywhere:
            mu[D + 1:], sg[D + 1:] = (h0 - span / 30.0)[D + 1:], (span / 6.0)[D + 1:]
            df[D + 1:] = 0.0 if prior == "gauss" else 3.0
            if prior == "mixed":
                df[D + 1::2] = 0.0
        hprior = {"mu": mu, "sigma": sg, "df": df}
    Nnoise = (nf[0] == 1) + (nf[1] == 2) + 2 * (nf[2] == 1)
    gp = {"X": X, "y": y, "s2": s2, "covfun": 1, "Ncov": D + 1, "noisefun": nf, "Nnoise": Nnoise, "meanfun": meanfun,
          "Nmean": Nhyp - D - 1 - Nnoise, "intmeanfun": 0, "meanfun_extras": None}
    return dict(gp=gp, h0=h0, LB=LB, UB=UB, PLB=PLB, PUB=PUB, hprior=hprior)


# Parity cases: (seed, meanfun, noisefun, prior, fixed coordinate, coordinate with infinite bounds, TolFun, MaxIter[, D, N[, Ninit, Nopts]]);
# D = 2, N = 30, Ninit = PARITY_NINIT, Nopts = PARITY_NOPTS unless given.
# A quasi-Newton trajectory amplifies rounding-level differences between two correct evaluations of the objective, some problems by
# many orders of magnitude within forty iterations (the meanfun-4 problems here: 1e-13 in the gradient becomes 1e-6 in the iterate),
# and no implementation can then be pinned to the restatement at 1e-9.  The cases are therefore chosen ON THE CPU, with the oracle's
# gplite_nlZ as the objective, under two conditions that tests/test_trainopt_restatement.py asserts:
#   1. no Armijo or stopping decision of the restatement lies within 1e-6 relative of flipping, no two fill values within 1e-6;
#   2. a relative perturbation of 1e-13 of every gradient the objective returns (450 units of roundoff) moves no iterate of the
#      restatement by more than 1e-10: a factor of ten below the 1e-9 the device is held to.
# The D = 2 meanfun-4 cases meet 2. only over their first eight iterations (MaxIter = 8: they end with exit flag 0); case 7 is a
# one-dimensional meanfun-4 problem whose two starts run to exit flag 2.
#
# The WIDE cases (8 on) take the kernels' strided loops on their second trip and the factorisation through the forms that N, Nopts and
# Ninit select; MaxIter is small because condition 2. holds only that long (the starts end with exit flag 0, some of case 14's with
# 2).  Their recorded values are also held to the ORACLE at 1e-10 (tests/test_gpu_trainopt.py), which asks a third condition of them:
#   3. rounding the training inputs by one unit in the last place (a relative 2^-52 perturbation, two draws) moves the oracle's own
#      value at no iterate by more than 1e-11: the yardstick is settled a factor of ten below what it measures.
# "moved" is the largest movement of an iterate under the perturbation of 2., measured with the oracle when the case was chosen:
#   8-10  Nhyp = 3 D + 3 = 66 > 64: the one-wave loops of k_topt_decide (H y, -H_FF g_F, the Nhyp^2 update) and of the hyper-prior in
#         gpobj_emit beyond lane 63.  MaxIter 4: the first iteration steps along the gradient, the second scales H and updates it, from
#         the third on the direction is a full H product.  8: prior on the covariance parameters (moved 1.3e-11); 9: a Gaussian /
#         Student-t prior on EVERY coordinate, so that the prior's value and gradient beyond index 63 count (1.8e-12); 10: Student-t
#         everywhere and coordinate 64 (a length scale of the mean function) fixed: y_i = 0, the free set and the closing clamp on the
#         second trip (1.1e-12)
#   11    N = 300 with s2: sn2 / dsn2 / the minimum that picks the Cholesky branch beyond a workgroup's 256 threads, different per
#         point (5.4e-12)
#   12-13 N = 565: past 512 (k_alpha_solve, k_tri_inverse2<8>) and 560 (two Cholesky panels); output-dependent noise (two dsn2 rows per
#         point, 1.1e-12) and scaled s2 (3.0e-12)
#   14    Nopts = 16 at N = 200: 16 * 4 * 5 / 2 = 160 > 128 tiles, syrk_form 2; sixteen starts in lock-step.  TolFun 0.1: start 0 stops
#         after two iterations by the |df| rule, six more by it after three, the rest at MaxIter, so starts finish in different
#         rounds with different flags (1.1e-12).  Seed 11 was passed over: its last start runs the signal variance onto its upper
#         bound, cond(K + diag(sn2)) = 1.6e8 at its third iterate, where 3. fails (the oracle's value moves by 1.3e-9; the device's
#         value there was 7e-10 from the oracle's).  The noise model carries s2 >= 0.01 ON PURPOSE.  With noisefun (1,0,0) row 6 of the
#         design has a noise variance of 1.7e-5 against a signal variance of 11: cond(K + sn2 I) = 6.9e7, and rounding one unit in the
#         last place of the training inputs moves the ORACLE's fill value of that row by 1.1e-10 relative, more than TOL_FILL.  On the
#         device the batched fill stage and the single gplite_nlZ that drives the restatement, which agree to the last bit or two on
#         the other 23 rows, came out 1.8e-10 and 4.1e-11 from the oracle on that row and 2.2e-10 from each other: two correct
#         evaluations that TOL_FILL cannot tell apart from a wrong one.  With s2 the same perturbation moves no fill value by more
#         than 2.2e-13.
#   15    Ninit = 300: a second, ragged fill chunk (256 + 44), a ranking over more than 256 rows, M = 297 > 256 candidates for the
#         low-noise start; smallest fill gap 7.9e-4 (3.5e-11)
#   16    Ninit = 1024, the library's default: four full chunks; smallest fill gap 5.8e-4 (7.8e-13)
# Seen on an MI355X when the cases went in (fill error / smallest decision margin of the device-driven run / largest error of an iterate /
# recorded values against the oracle): 8: 0 / 1.0 / 3.1e-14 / 2.0e-15; 9: 1.7e-16 / 1.0 / 2.7e-15 / 1.1e-14; 10: 2.2e-16 / 1.0 /
# 1.2e-15 / 2.0e-14; 11: 6.0e-16 / 0.97 / 1.2e-11 / 2.2e-13; 12: 6.0e-15 / 0.99 / 1.3e-12 / 6.2e-13; 13: 1.0e-14 / 0.97 / 6.8e-12 /
# 5.4e-13; 14: 1.3e-15 / 1.2e-2 / 1.2e-12 / 2.1e-13; 15: 2.3e-11 / 0.95 / 7.9e-11 / 4.5e-12; 16: 4.0e-11 / 0.97 / 3.5e-13 / 3.0e-13.
PARITY_CASES = [
    (40, 4, (1, 0, 0), "flat", None, None, 1e-4, 8),
    (12, 0, (1, 1, 0), "gauss", None, None, 1e-4, 1000),
    (13, 1, (1, 2, 0), "student", 0, None, 1e-3, 1000),
    (11, 1, (1, 0, 1), "mixed", None, 2, 1e-4, 1000),
    (15, 1, (1, 0, 0), "student", 1, 2, 1e-4, 1000),
    (11, 0, (1, 0, 0), "flat", 1, None, 1e-4, 1000),
    (40, 4, (1, 0, 0), "gauss", None, None, 1e-4, 8),
    (11, 4, (1, 0, 0), "gauss", None, None, 1e-3, 1000, 1, 40),     # D = 1, N = 40: a meanfun-4 problem that meets 2. up to its stopping test
    (41, 4, (1, 0, 0), "gauss", None, None, 1e-4, 4, 21, 70),
    (41, 4, (1, 0, 0), "mixed-all", None, None, 1e-4, 4, 21, 70),
    (41, 4, (1, 0, 0), "student-all", 64, None, 1e-4, 4, 21, 70),
    (11, 1, (1, 1, 0), "student", None, None, 1e-4, 6, 3, 300),
    (12, 1, (1, 0, 1), "flat", None, None, 1e-4, 4, 3, 565),
    (12, 1, (1, 2, 0), "flat", None, None, 1e-4, 4, 3, 565),
    (12, 1, (1, 1, 0), "student", None, None, 1e-1, 3, 2, 200, 24, 16),
    (11, 1, (1, 0, 0), "gauss", None, None, 1e-4, 6, 2, 30, 300, 3),
    (11, 1, (1, 0, 0), "gauss", None, None, 1e-4, 3, 2, 30, 1024, 3),
]
PARITY_NINIT, PARITY_NOPTS = 24, 2
WIDE_CASES = range(8, len(PARITY_CASES))


def parity_case(ci):
    seed, mf, nf, pr, fx, ib, tol, maxit = PARITY_CASES[ci][:8]
    D, N = PARITY_CASES[ci][8:10] or (2, 30)
    return gp_case(seed, D=D, N=N, meanfun=mf, noisefun=nf, prior=pr, fixed=fx, infbound=ib), tol, maxit


def parity_sizes(ci):
    """(Ninit, Nopts) of a parity case"""
    return PARITY_CASES[ci][10:12] or (PARITY_NINIT, PARITY_NOPTS)


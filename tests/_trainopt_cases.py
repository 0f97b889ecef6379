"""Small GP training problems shared by the CPU and the GPU tests of the optimisation half of gplite_train."""
import numpy as np


def gp_case(seed, D=2, N=30, meanfun=4, noisefun=(1, 0, 0), prior="flat", fixed=None, infbound=None):
    """A dict: gp (the struct gplite_nlZ reads), h0, LB, UB, PLB, PUB, hprior (None for a flat prior)."""
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
    if fixed is not None:
        LB[fixed] = UB[fixed] = PLB[fixed] = PUB[fixed] = h0[fixed]
    if infbound is not None:
        LB[infbound], UB[infbound] = -np.inf, np.inf
    Nhyp = h0.size
    hprior = None
    if prior != "flat":
        mu, sg, df = np.full(Nhyp, np.nan), np.full(Nhyp, np.nan), np.full(Nhyp, np.nan)
        mu[:D + 1], sg[:D + 1] = h0[:D + 1] + 0.2, 1.5
        df[:D + 1] = 0.0 if prior == "gauss" else 3.0
        if prior == "mixed":
            df[0] = 0.0
        hprior = {"mu": mu, "sigma": sg, "df": df}
    Nnoise = (nf[0] == 1) + (nf[1] == 2) + 2 * (nf[2] == 1)
    gp = {"X": X, "y": y, "s2": s2, "covfun": 1, "Ncov": D + 1, "noisefun": nf, "Nnoise": Nnoise, "meanfun": meanfun,
          "Nmean": Nhyp - D - 1 - Nnoise, "intmeanfun": 0, "meanfun_extras": None}
    return dict(gp=gp, h0=h0, LB=LB, UB=UB, PLB=PLB, PUB=PUB, hprior=hprior)


# Parity cases: (seed, meanfun, noisefun, prior, fixed coordinate, coordinate with infinite bounds, TolFun, MaxIter[, D, N]); D = 2, N = 30
# unless given.
# A quasi-Newton trajectory amplifies rounding-level differences between two correct evaluations of the objective, some problems by
# many orders of magnitude within forty iterations (the meanfun-4 problems here: 1e-13 in the gradient becomes 1e-6 in the iterate),
# and no implementation can then be pinned to the restatement at 1e-9.  The cases are therefore chosen ON THE CPU, with the oracle's
# gplite_nlZ as the objective, under two conditions that tests/test_trainopt_restatement.py asserts:
#   1. no Armijo or stopping decision of the restatement lies within 1e-6 relative of flipping, no two fill values within 1e-6;
#   2. a relative perturbation of 1e-13 of every gradient the objective returns (450 units of roundoff) moves no iterate of the
#      restatement by more than 1e-10: a factor of ten below the 1e-9 the device is held to.
# The D = 2 meanfun-4 cases meet 2. only over their first eight iterations (MaxIter = 8: they end with exit flag 0); the last case is a
# one-dimensional meanfun-4 problem whose two starts run to exit flag 2.
PARITY_CASES = [
    (40, 4, (1, 0, 0), "flat", None, None, 1e-4, 8),
    (12, 0, (1, 1, 0), "gauss", None, None, 1e-4, 1000),
    (13, 1, (1, 2, 0), "student", 0, None, 1e-3, 1000),
    (11, 1, (1, 0, 1), "mixed", None, 2, 1e-4, 1000),
    (15, 1, (1, 0, 0), "student", 1, 2, 1e-4, 1000),
    (11, 0, (1, 0, 0), "flat", 1, None, 1e-4, 1000),
    (40, 4, (1, 0, 0), "gauss", None, None, 1e-4, 8),
    (11, 4, (1, 0, 0), "gauss", None, None, 1e-3, 1000, 1, 40),     # D = 1, N = 40: a meanfun-4 problem that meets 2. up to its stopping test
]
PARITY_NINIT, PARITY_NOPTS = 24, 2


def parity_case(ci):
    seed, mf, nf, pr, fx, ib, tol, maxit = PARITY_CASES[ci][:8]
    D, N = PARITY_CASES[ci][8:] or (2, 30)
    return gp_case(seed, D=D, N=N, meanfun=mf, noisefun=nf, prior=pr, fixed=fx, infbound=ib), tol, maxit

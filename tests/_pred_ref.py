"""Extended-precision restatement of the GP prediction and of the Bayesian quadrature, and test points that see the data
(test infrastructure).

``pred_ld(gp, Xs, ys, s2s)`` restates gplite/gplite_pred.m:73-121 and ``quad_ld(gp, mu, sigma)`` gplite/gplite_quad.m:70-106 in
``numpy.longdouble`` (64-bit mantissa) from the gp dict's own float64 ``X``, ``hyp``, ``alpha``, ``L``, ``sW``: plain coordinate
differences for the distances (no centring, no |a|^2 + |b|^2 - 2 a.b), ``exp``, and forward substitution row by row for the Cholesky
samples.  Nothing is clamped inside: ``fs2`` / ``varF`` come back as computed, the caller applies ``max(., 0)`` / ``max(., eps)``.

``near_data_points`` draws test points at a chosen kernel value from a training input, whatever D is: with the recipe of
tests/_cases.synth_problem (points 1.3 N(0, I) around inputs 1.5 N(0, I), length scales 0.8) the cross-kernel is numerically zero
from D = 13 upwards, and a prediction test then compares the mean function and sf2.  ``power`` says, from the reference alone, how much
of a point set sees the data; ``POWER_V`` / ``POWER_M`` are the shares every prediction case has to reach.

The error measures (``err_fs2``, ``err_fmu``) are in units of u = 2^-53 of the magnitudes that are actually added up:
    fs2, ys2, varF:  |got - ref| / (u (kss + vmag)),   vmag = sum V.^2 (Cholesky samples) or |Ks|' |L| |Ks| (low-noise samples)
    fmu, F:          |got - ref| / (u (|m*| + sum_n |Ks_n alpha_n|))
"""
import math
from collections import namedtuple

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is no wider than float64 here: the restatement would be no reference"
U = 2.0 ** -53
EPS = 2.0 ** -52
POWER_V, POWER_M, POWER_OK = 0.5, 0.9, 0.9   # shares of pairs that see the data; of acquisition points inside the `ok` mask

# fmu / fs2 / ys2: Nstar x S longdouble, unclamped.  sn2s: the noise term of ys2 (ys2 = fs2 + sn2s).  kss: S (sf2, or nf_kk for the
# quadrature).  expl = kss - fs2: the variance the data explain (sum V.^2).  vmag, fmag: the magnitudes of the error measures.
# data = Ks' alpha: fmu's data term.
PredLD = namedtuple("PredLD", "fmu fs2 ys2 sn2s kss expl vmag fmag data")


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _meanfun_ld(gp, hyp, Xs):
    """gplite_meanfun.m:398-436 for the ids 0, 1, 4"""
    D = Xs.shape[1]
    hm = hyp[gp["Ncov"] + gp["Nnoise"]:]
    if gp["meanfun"] == 0:
        return np.zeros(Xs.shape[0], dtype=LD)
    if gp["meanfun"] == 1:
        return hm[0] * np.ones(Xs.shape[0], dtype=LD)
    assert gp["meanfun"] == 4
    xm, omega = hm[1:D + 1], np.exp(hm[D + 1:2 * D + 1])
    return hm[0] - LD(0.5) * np.sum(((Xs - xm[None, :]) / omega[None, :]) ** 2, axis=1)


def _noise_ld(gp, hyp, Nstar, ys, s2s):
    """gplite_noisefun.m:176-207 at the test points: an empty s2star counts as zero, the output-dependent term needs a ystar"""
    nf = tuple(gp["noisefun"]) + (0,) * (3 - len(gp["noisefun"]))
    hn = hyp[gp["Ncov"]:gp["Ncov"] + gp["Nnoise"]]
    i = 0
    sn2 = np.full(Nstar, LD(EPS))
    if nf[0] == 1:
        sn2 = np.full(Nstar, np.exp(2 * hn[i]))
        i += 1
    s2 = np.zeros(Nstar, dtype=LD) if s2s is None else _ld(s2s).reshape(-1)
    if nf[1] == 1:
        sn2 = sn2 + s2
    elif nf[1] == 2:
        sn2 = sn2 + np.exp(hn[i]) * s2
        i += 1
    if nf[2] == 1 and ys is not None:
        zz = np.maximum(LD(0), hn[i] - _ld(ys).reshape(-1))
        sn2 = sn2 + np.exp(2 * hn[i + 1]) * zz ** 2
    return sn2


def _fwd(R, B):
    """R' \\ B for an upper-triangular R, row by row"""
    V = np.empty_like(B)
    for i in range(B.shape[0]):
        V[i] = (B[i] - R[:i, i] @ V[:i]) / R[i, i]
    return V


def _variance_terms(post, Ks):
    """-> (expl, vmag) of one hyper-sample for the N x Nstar cross-kernel Ks: gplite_pred.m:99-104"""
    L = _ld(post["L"])
    if post["Lchol"]:
        V = _fwd(L, _ld(post["sW"])[:, None] * Ks)          # :99
        expl = np.sum(V * V, axis=0)                         # :100
        return expl, expl
    expl = -np.sum(Ks * (L @ Ks), axis=0)                    # :103-104, L = -inv(K + sn2 I)
    return expl, np.sum(np.abs(Ks) * (np.abs(L) @ np.abs(Ks)), axis=0)


def pred_ld(gp, Xs, ys=None, s2s=None):
    X, Xs = _ld(gp["X"]), _ld(Xs)
    (N, D), Nstar, S = X.shape, Xs.shape[0], len(gp["post"])
    out = {k: np.zeros((Nstar, S), dtype=LD) for k in ("fmu", "fs2", "ys2", "sn2s", "expl", "vmag", "fmag", "data")}
    kss = np.zeros(S, dtype=LD)
    for s, post in enumerate(gp["post"]):
        hyp = _ld(post["hyp"])
        ell, sf2 = np.exp(hyp[:D]), np.exp(2 * hyp[D])
        d2 = np.zeros((N, Nstar), dtype=LD)
        for d in range(D):
            d2 += ((X[:, d][:, None] - Xs[:, d][None, :]) / ell[d]) ** 2
        Ks = sf2 * np.exp(-d2 / 2)                                                   # :73-74
        alpha = _ld(post["alpha"]).reshape(-1)
        mstar = _meanfun_ld(gp, hyp, Xs)
        out["data"][:, s] = Ks.T @ alpha
        out["fmu"][:, s] = mstar + out["data"][:, s]                                 # :83
        out["fmag"][:, s] = np.abs(mstar) + np.abs(Ks).T @ np.abs(alpha)
        out["expl"][:, s], out["vmag"][:, s] = _variance_terms(post, Ks)
        out["fs2"][:, s] = sf2 - out["expl"][:, s]                                   # :100,:104 (before :120's clamp)
        out["sn2s"][:, s] = _noise_ld(gp, hyp, Nstar, ys, s2s) * LD(post["sn2_mult"])
        out["ys2"][:, s] = out["fs2"][:, s] + out["sn2s"][:, s]                      # :121
        kss[s] = sf2
    return PredLD(kss=kss, **out)


def quad_ld(gp, mu, sigma):
    """F / varF per hyper-sample in the fields fmu / fs2 (ys2 repeats fs2, sn2s is zero); kss holds nf_kk"""
    X, mu = _ld(gp["X"]), _ld(mu)
    (N, D), Nstar, S = X.shape, mu.shape[0], len(gp["post"])
    sigma = _ld(sigma).reshape(-1)
    assert sigma.shape == (D,) and gp["meanfun"] in (0, 1, 4) and tuple(gp["noisefun"])[:3] in ((1, 0, 0), (1, 0))
    out = {k: np.zeros((Nstar, S), dtype=LD) for k in ("fmu", "fs2", "ys2", "sn2s", "expl", "vmag", "fmag", "data")}
    kss = np.zeros(S, dtype=LD)
    Ncov, Nnoise = gp["Ncov"], gp["Nnoise"]
    for s, post in enumerate(gp["post"]):
        hyp = _ld(post["hyp"])
        ell, ln_sf2, sum_lnell = np.exp(hyp[:D]), 2 * hyp[D], np.sum(hyp[:D])        # :42-44
        tau = np.sqrt(sigma ** 2 + ell ** 2)                                         # :70
        lnnf = ln_sf2 + sum_lnell - np.sum(np.log(tau))                              # :71
        d2 = np.zeros((N, Nstar), dtype=LD)
        for d in range(D):                                                           # :72-75
            d2 += ((X[:, d][:, None] - mu[:, d][None, :]) / tau[d]) ** 2
        z = np.exp(lnnf - d2 / 2)                                                    # :76 (N x Nstar)
        alpha = _ld(post["alpha"]).reshape(-1)
        m = np.full(Nstar, hyp[Ncov + Nnoise] if gp["meanfun"] > 0 else LD(0))       # :47
        if gp["meanfun"] == 4:                                                       # :79-82
            xm, omega = hyp[Ncov + Nnoise + 1:Ncov + Nnoise + 1 + D], np.exp(hyp[Ncov + Nnoise + D + 1:Ncov + Nnoise + 2 * D + 1])
            m = m - LD(0.5) * np.sum((mu ** 2 + sigma[None, :] ** 2 - 2 * mu * xm[None, :] + xm[None, :] ** 2) / omega[None, :] ** 2, axis=1)
        out["data"][:, s] = z.T @ alpha
        out["fmu"][:, s] = out["data"][:, s] + m                                     # :77,:82
        out["fmag"][:, s] = np.abs(m) + np.abs(z).T @ np.abs(alpha)
        nf_kk = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(np.sqrt(2 * sigma ** 2 + ell ** 2))))    # :98-99
        if post["Lchol"]:                                                            # :101: z' inv(L'L) z / sn2_eff = |L' \ z|^2 / sn2_eff
            sn2_eff = np.exp(2 * hyp[Ncov]) * LD(post["sn2_mult"])                   # :66-67
            V = _fwd(_ld(post["L"]), z)
            expl = np.sum(V * V, axis=0) / sn2_eff
            vmag = expl
        else:
            expl, vmag = _variance_terms(post, z)                                    # :103
        out["expl"][:, s], out["vmag"][:, s] = expl, vmag
        out["fs2"][:, s] = nf_kk - expl                                              # :105 (before :106's clamp)
        out["ys2"][:, s] = out["fs2"][:, s]
        kss[s] = nf_kk
    return PredLD(kss=kss, **out)


def mean_lengthscales(gp):
    D = gp["X"].shape[1]
    return np.mean(np.stack([np.exp(np.asarray(p["hyp"][:D], dtype=np.float64)) for p in gp["post"]], axis=1), axis=1)


def near_data_points(gp, Nstar, rng, lo=1e-2, hi=0.999, exact=0.0, far=0.0, scale=None):
    """Nstar points x* = X[i] + ell (.) u sqrt(-2 ln rho): i uniform over the training inputs, u uniform on the sphere, rho log-uniform
    in [lo, hi], ell the mean length scales over the hyper-samples (``scale`` replaces it: the quadrature's tau).  k(x*, X_i) / sf2 is
    then about rho at every D.  ``exact``: the share that are training inputs themselves (fs2 cancels in full); ``far``: the share
    drawn 1.3 N(0, I), the recipe that sees no data at large D.  The three kinds are shuffled, so that they meet in the 16-point tiles."""
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    ell = mean_lengthscales(gp) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    n_exact, n_far = int(exact * Nstar), int(far * Nstar)
    n_near = Nstar - n_exact - n_far
    u = rng.standard_normal((n_near, D))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rho = np.exp(rng.uniform(math.log(lo), math.log(hi), size=n_near))
    near = X[rng.integers(0, N, size=n_near)] + ell[None, :] * u * np.sqrt(-2.0 * np.log(rho))[:, None]
    pts = np.vstack([near, X[rng.integers(0, N, size=n_exact)], 1.3 * rng.standard_normal((n_far, D))])
    return np.ascontiguousarray(pts[rng.permutation(Nstar)])


def power_of(ref):
    """-> (share of (point, sample) pairs with explained variance > 1e-3 kss, share with |data term| > 1e-3 |fmu|) of a PredLD"""
    return (float(np.mean(ref.expl > 1e-3 * ref.kss[None, :])), float(np.mean(np.abs(ref.data) > 1e-3 * np.abs(ref.fmu))))


def power(gp, Xs):
    return power_of(pred_ld(gp, Xs))


def assert_power(ref, what=""):
    pv, pm = power_of(ref)
    assert pv >= POWER_V and pm >= POWER_M, "%s: the points do not see the data: shares %.3f (variance), %.3f (mean)" % (what, pv, pm)
    return pv, pm


def err_fs2(got, ref, clamp=0.0, field="fs2"):
    """worst |got - max(ref, clamp)| / (u (kss + vmag)); ``field`` "ys2" adds the noise term to the reference after the clamp"""
    want = np.maximum(ref.fs2, LD(clamp)) + (ref.sn2s if field == "ys2" else 0)
    return float(np.max(np.abs(_ld(got).reshape(want.shape) - want) / (U * (ref.kss[None, :] + ref.vmag))))


def err_fmu(got, ref):
    return float(np.max(np.abs(_ld(got).reshape(ref.fmu.shape) - ref.fmu) / (U * ref.fmag)))

"""The HOST forms of the Gaussian-mixture variational posterior in the transformed space: the draw, the analytic moments and the log
density, in NumPy.  The device forms, which also cover the caller's own parameter space, are vptools.vbmc_rnd / vbmc_moments /
vbmc_pdf; ``vbmc_amd.vbmc_rnd`` and ``vbmc_amd.vbmc_moments`` are the host forms of this module.
"""
from __future__ import annotations

import numpy as np

from ._lib import VbmcUnsupported


def vbmc_rnd(vp, N, origflag=False, balanceflag=False, *, rng=None):
    """[X,I] = vbmc_rnd(vp,N,0,balanceflag)  (vbmc_rnd.m:50-109): N draws from the Gaussian-mixture variational
    posterior in the TRANSFORMED space, on the HOST with a NumPy ``rng`` (origflag must be false here; the device form, with the variable
    transform and ``seed=`` / ``block=``, is vptools.vbmc_rnd).  Places the importance points of the IQR acquisition functions."""
    if origflag:
        raise VbmcUnsupported(-1, "vbmc_rnd: origflag = 1 needs warpvars_vbmc (caller's side)")
    rng = np.random.default_rng() if rng is None else rng
    D, K = int(vp["D"]), int(vp["K"])
    N = int(N)
    if N < 1:
        return np.zeros((0, D)), np.zeros(0, dtype=int)
    w = np.asarray(vp["w"], dtype=np.float64).reshape(K)
    mu_t = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K).T
    sigma = np.asarray(vp["sigma"], dtype=np.float64).reshape(K)
    lam = np.asarray(vp["lambda"], dtype=np.float64).reshape(D)
    if K > 1:
        if balanceflag:                                       # exact split by weight + weighted remainder (:69-88)
            n_floor = np.floor(w * N).astype(int)
            I = np.repeat(np.arange(K), n_floor)
            if N > I.size:
                w_extra = w * N - n_floor
                n_extra = int(np.ceil(np.sum(w_extra)))
                w_extra = w_extra + w * (n_extra - np.sum(w_extra))
                I = np.concatenate([I, rng.choice(K, size=n_extra, p=w_extra / np.sum(w_extra))])
            I = I[rng.permutation(I.size)[:N]]
        else:
            I = rng.choice(K, size=N, p=w / np.sum(w))        # catrnd(w,N) (:90)
        X = mu_t[I] + lam[None, :] * (rng.standard_normal((N, D)) * sigma[I][:, None])      # :95
    else:
        I = np.zeros(N, dtype=int)
        X = mu_t + lam[None, :] * (rng.standard_normal((N, D)) * sigma[0])                   # :103
    return X, I


def vbmc_moments(vp, origflag=False):
    """[mubar,Sigma] = vbmc_moments(vp,0)  (vbmc_moments.m:30-43): mean and covariance of the Gaussian-mixture variational posterior
    in the TRANSFORMED space, analytically on the HOST (origflag = 1 samples through the variable transform: the device form
    vptools.vbmc_moments)."""
    if origflag:
        raise VbmcUnsupported(-1, "vbmc_moments: origflag = 1 needs warpvars_vbmc (caller's side)")
    D, K = int(vp["D"]), int(vp["K"])
    w = np.asarray(vp["w"], dtype=np.float64).reshape(1, K)
    mu = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)
    sigma = np.asarray(vp["sigma"], dtype=np.float64).reshape(1, K)
    lam = np.asarray(vp["lambda"], dtype=np.float64).reshape(D)
    mubar = np.sum(w * mu, axis=1)
    Sigma = np.sum(w * sigma ** 2) * np.diag(lam ** 2)
    for k in range(K):
        dk = (mu[:, k] - mubar).reshape(D, 1)
        Sigma = Sigma + w[0, k] * (dk @ dk.T)
    return mubar, Sigma


def vbmc_lnpdf(vp, X):
    """log vbmc_pdf(vp,X,0,1) in the transformed space (vbmc_pdf.m:38-71 with logflag): Gaussian mixture on the HOST
    (Na x K); the device form, either space, is vptools.vbmc_pdf."""
    X = np.asarray(X, dtype=np.float64)
    D, K = int(vp["D"]), int(vp["K"])
    mu = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)
    sigma = np.asarray(vp["sigma"], dtype=np.float64).reshape(K)
    lam = np.asarray(vp["lambda"], dtype=np.float64).reshape(D)
    w = np.asarray(vp["w"], dtype=np.float64).reshape(K)
    z = (X[:, None, :] - mu.T[None, :, :]) / (lam[None, None, :] * sigma[None, :, None])
    lp = np.log(w)[None, :] - 0.5 * np.sum(z * z, axis=2) - D * np.log(sigma)[None, :] - np.sum(np.log(lam)) - 0.5 * D * np.log(2 * np.pi)
    m = np.max(lp, axis=1, keepdims=True)
    out = (m + np.log(np.sum(np.exp(lp - m), axis=1, keepdims=True))).reshape(-1)
    # the reference forms the density and then takes its log (vbmc_pdf.m:71,117): below the smallest double it is log(0) = -Inf
    return np.where(out < np.log(5e-324), -np.inf, out)

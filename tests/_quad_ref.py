"""NumPy restatement of the reference's Bayesian quadrature for a GP and of the acquisition wrapper's vp.delta branch (test infrastructure).

``gplite_quad(gp, mu, sigma, ssflag, nargout)`` restates gplite/gplite_quad.m:1-119 for the mean functions 0 (zero), 1 (constant) and
4 (negative quadratic) line by line, with the reference's orders of summation; ``gp`` is the dict of oracle/vbmc_ref.py (``post`` holds
hyp, alpha, L, Lchol, sn2_mult per hyper-sample).  ``acqwrapper_vbmc(Xs, vp, gp, optimState, acq_name, outside)`` restates
acq/acqwrapper_vbmc.m:11-52 with any(vp.delta > 0): the per-hyper-sample mean and variance come from gplite_quad(gp,Xs,vp.delta',1) (:12-14),
everything behind them from the oracle's own acquisition formulas.
"""
import glob
import json
import math
import os

import numpy as np

from oracle import vbmc_ref as R

EPS = 2.0 ** -52   # MATLAB's eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gplite_quad(gp, mu, sigma, ssflag=False, nargout=2):
    """-> (F, varF): Nstar x S with ssflag or S == 1 (the reference's Nstar x Ns), Nstar vectors otherwise; varF None for nargout < 2."""
    compute_var = nargout > 1                                                   # :6
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape                                                              # :8
    Ns = len(gp["post"])                                                        # :9
    Ncov, Nnoise = gp["Ncov"], gp["Nnoise"]                                     # :12-13
    if gp["meanfun"] not in (0, 1, 4):                                          # :16-19 (6 and 8 are not restated)
        raise NotImplementedError("gplite_quad:UnsupportedMeanFun")
    if gp.get("covfun", 1) != 1:                                                # :21-24
        raise NotImplementedError("gplite_quad:UnsupportedCovFun")
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, D)
    Nstar = mu.shape[0]                                                         # :26
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1, D)
    if sigma.shape[0] == 1:
        sigma = np.repeat(sigma, Nstar, axis=0)                                 # :27
    quadratic_meanfun = gp["meanfun"] == 4                                      # :30
    F = np.zeros((Nstar, Ns))                                                   # :34
    varF = np.zeros((Nstar, Ns)) if compute_var else None                       # :35
    for s, post in enumerate(gp["post"]):                                       # :38
        hyp = np.asarray(post["hyp"], dtype=np.float64)                         # :39
        ell = np.exp(hyp[0:D])[None, :]                                         # :42
        ln_sf2 = 2.0 * hyp[D]                                                   # :43
        sum_lnell = np.sum(hyp[0:D])                                            # :44
        m0 = hyp[Ncov + Nnoise] if gp["meanfun"] > 0 else 0.0                   # :47
        if quadratic_meanfun:
            xm = hyp[Ncov + Nnoise + 1:Ncov + Nnoise + 1 + D][None, :]          # :49
            omega = np.exp(hyp[Ncov + Nnoise + D + 1:Ncov + Nnoise + 2 * D + 1])[None, :]   # :50
        alpha = np.asarray(post["alpha"], dtype=np.float64).reshape(-1)         # :62
        L = np.asarray(post["L"], dtype=np.float64)                             # :63
        Lchol = bool(post["Lchol"])                                             # :64
        sn2 = math.exp(2.0 * hyp[Ncov])                                         # :66
        sn2_eff = sn2 * post["sn2_mult"]                                        # :67
        tau = np.sqrt(sigma ** 2 + ell ** 2)                                    # :70
        lnnf = ln_sf2 + sum_lnell - np.sum(np.log(tau), axis=1)                 # :71
        sumdelta2 = np.zeros((Nstar, N))                                        # :72
        for i in range(D):                                                      # :73-75
            sumdelta2 = sumdelta2 + ((mu[:, i][:, None] - X[:, i][None, :]) / tau[:, i][:, None]) ** 2
        z = np.exp(lnnf[:, None] - 0.5 * sumdelta2)                             # :76
        F[:, s] = z @ alpha + m0                                                # :77
        if quadratic_meanfun:                                                   # :79-82
            nu_k = -0.5 * np.sum(1.0 / omega ** 2 * (mu ** 2 + sigma ** 2 - 2 * mu * xm + xm ** 2), axis=1)
            F[:, s] = F[:, s] + nu_k
        if compute_var:                                                         # :97
            tau_kk = np.sqrt(2 * sigma ** 2 + ell ** 2)                         # :98
            nf_kk = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tau_kk), axis=1))  # :99
            if Lchol:
                invKzk = R.solve_upper(L, R.solve_upper_t(L, z.T)) / sn2_eff    # :101
            else:
                invKzk = -L @ z.T                                               # :103
            J_kk = nf_kk - np.sum(z * invKzk.T, axis=1)                         # :105
            varF[:, s] = np.maximum(EPS, J_kk)                                  # :106
    if Ns > 1 and not ssflag:                                                   # :112
        Fbar = np.sum(F, axis=1) / Ns                                           # :113
        if compute_var:
            varFss = np.sum((F - Fbar[:, None]) ** 2, axis=1) / (Ns - 1)        # :115
            varF = np.sum(varF, axis=1) / Ns + varFss                           # :116
        F = Fbar                                                                # :118
    return F, varF


def nf_kk(gp, sigma):
    """nf_kk per hyper-sample (:98-99): the scale of varF."""
    D = gp["X"].shape[1]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    return np.array([math.exp(2.0 * p["hyp"][D] + np.sum(p["hyp"][:D]) - np.sum(np.log(np.sqrt(2 * sigma ** 2 + np.exp(p["hyp"][:D]) ** 2))))
                     for p in gp["post"]])


def acqwrapper_vbmc(Xs, vp, gp, optimState, acq_name, outside=None):
    """acq/acqwrapper_vbmc.m:11-52 with any(vp.delta > 0), without the integer mapping (:8) and with the hard-bound test (:49-52)
    supplied as the boolean mask ``outside`` -> (acq, fbar, vtot)."""
    Xs = np.asarray(Xs, dtype=np.float64)
    delta = np.asarray(vp["delta"], dtype=np.float64).reshape(-1)
    assert np.any(delta > 0)                                                    # :12
    fmu, fs2 = gplite_quad(gp, Xs, delta[None, :], True)                        # :14
    Ns = fmu.shape[1]                                                           # :21
    fbar = np.sum(fmu, axis=1) / Ns                                             # :22
    vbar = np.sum(fs2, axis=1) / Ns                                             # :23
    vf = np.sum((fmu - fbar[:, None]) ** 2, axis=1) / (Ns - 1) if Ns > 1 else 0.0   # :24-28
    vtot = vf + vbar                                                            # :29
    acq = R.acq_function(acq_name, Xs, vp, gp, optimState, fmu, fs2, fbar, vtot)    # :32
    if optimState.get("VarianceRegularizedAcqFcn", False):                      # :35-46
        TolVar = optimState["TolGPVar"]
        idx = vtot < TolVar
        if np.any(idx):
            if R.ACQ_LOG_FLAG[acq_name]:
                acq[idx] = acq[idx] + TolVar / vtot[idx] - 1
            else:
                acq[idx] = acq[idx] * np.exp(-(TolVar / vtot[idx] - 1))
    acq = np.maximum(acq, -R.REALMAX)                                           # :47
    if outside is not None:
        acq = np.where(np.asarray(outside, dtype=bool), np.inf, acq)            # :50-52
    return acq, fbar, vtot


# ---- the 50-digit cases of tools/mp_quad_golden.py -----------------------------------------------------------------------------
def quad_golden_cases():
    return sorted(glob.glob(os.path.join(GOLDEN, "mp_quad_case*.json")))


def load_quad_golden(path):
    """-> (inputs dict of arrays, gp with the 50-digit alpha / L plugged in, expected dict of arrays)."""
    with open(path) as f:
        rec = json.load(f)
    inp = {k: (np.array(v, dtype=np.float64) if isinstance(v, list) else v) for k, v in rec["inputs"].items()}
    exp = {k: np.array(v, dtype=np.float64) for k, v in rec["expected"].items() if k != "Lchol"}
    gp = R.gplite_post(inp["hyp"], inp["X"], inp["y"], meanfun=inp["meanfun"])
    for s, post in enumerate(gp["post"]):
        assert post["Lchol"] == rec["expected"]["Lchol"][s] and post["sn2_mult"] == 1.0
        post["alpha"] = exp["alpha"][s]
        post["L"] = exp["L"][s]
    return inp, gp, exp


def mixed_gp(seed, D, N, S, meanfun, low_noise=True):
    """A seeded GP for the device tests: Cholesky samples at sn = 0.03 and, with ``low_noise`` and S > 1, the middle hyper-sample at
    sn2 = 9e-8 < 1e-6 (L = -inv(K + sn2 I), gplite_core.m:67,84-99), in one GP.  That sample's length scales are a quarter of the others':
    with next to no noise, close training inputs would make inv(K + sn2 I) -- and the rounding error of anything multiplied by it -- huge."""
    from tests._cases import synth_problem

    p = synth_problem(seed, D, N, 3, S, meanfun=meanfun)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(0.03)
    if low_noise and S > 1:
        hyp[D + 1, S // 2] = math.log(3e-4)
        hyp[:D, S // 2] += math.log(0.25)
    return R.gplite_post(hyp, p["X"], p["y"], meanfun=meanfun), p

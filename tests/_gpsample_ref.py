"""The surrogate sampler of vbmc_gp_surrogate_sample (include/vbmc_hip.h) restated in NumPy, and the shared case table of
tests/test_gpsample_restatement.py (CPU) and tests/test_gpu_gpsample.py.

The target is log_gpfun (gplite/gplite_sample.m:109-117) on the oracle's gplite_pred -- the noisy pair averaged over all hyper-samples
(gplite_pred.m:154-164) --, handed as the callable to tests/_issample_ref.py::sample, whose ``S`` axis is the ENSEMBLE here: E
independent ensembles on one target.  Restated beside it: the noise estimate (misc/gpsample_vbmc.m:30-38) and the interleave of the
records into the output rows (row e + E i is record i of ensemble e, rows >= Ns dropped).

Cases (D, N, S, E, W, Ns, thin, meanfun, low_noise, tight, VarThresh, beta, seed): the smallest shapes at which each piece can go wrong
  A  S = 1, VarThresh = Inf, beta = 0: the no-averaging branch and the mean-only target
  B  S = 3, meanfun 4, E = 2, thin 2, a finite VarThresh: the averaging with vy; the threshold active on some candidates and inactive
     on others; two ensembles that do not advance in step
  C  S = 2, one Lchol = false hyper-sample beside a Cholesky one, meanfun 1, beta = 0.5: the L branch and the beta term
  D  D = 32, W = 66: 198 candidates at spec 3 -- twelve full 16-point tiles and a partial one; QS = 8
  E  D = 1, E = 5, W = 4 (H = 2), Ns = 23, a tight box: outside proposals; Nm = 5 with two dropped rows in the interleave
  F  D = 1, N = 16, Ns = 300: more than the 256 records the IMIQR entry points allow
  G  N = 1136, S = 2 on both branches, Ns = 4: the top of the range in which inv(L') stays resident
"""
import math

import numpy as np

from oracle import vbmc_ref as R
from tests import _issample_ref as I

MARGIN = I.MARGIN
SLOTS = I.SLOTS
GAP = 1e-9

# name: (D, N, S, E, W, Ns, thin, meanfun, low_noise, tight, VarThresh, beta, seed)
CASES = {
    "A": (2, 33, 1, 1, 6, 40, 1, 0, False, False, np.inf, 0.0, 1),
    "B": (3, 40, 3, 2, 8, 24, 2, 4, False, False, 0.5, 0.0, 1),
    "C": (3, 40, 2, 1, 8, 10, 1, 1, True, False, np.inf, 0.5, 1),
    "D": (32, 40, 2, 1, 66, 8, 1, 4, False, False, np.inf, 0.0, 1),
    "E": (1, 20, 1, 5, 4, 23, 1, 0, False, True, np.inf, 0.0, 1),
    "F": (1, 16, 1, 1, 4, 300, 1, 0, False, False, np.inf, 0.0, 1),
    "G": (3, 1136, 2, 1, 8, 4, 1, 1, True, False, np.inf, 0.0, 1),
}


def burnin_of(Ns):
    return int(math.ceil(Ns / 5))                      # gplite_sample.m:71


def log_gpfun(gp, VarThresh, beta, stats=None):
    """logp(P, e): log_gpfun of gplite_sample.m:109-117 on the oracle's averaged prediction; ``stats`` counts the evaluated points on
    which the threshold acted and those on which it did not"""
    plain = (VarThresh == 0 or not np.isfinite(VarThresh)) and beta == 0

    def logp(P, e):
        ymu, ys2, _, _ = R.gplite_pred(gp, P)
        y, s2 = np.array(ymu, dtype=np.float64).reshape(-1), np.asarray(ys2, dtype=np.float64).reshape(-1)
        if plain:
            return y
        over = s2 >= VarThresh
        if stats is not None:
            stats["active"] += int(np.sum(over))
            stats["inactive"] += int(np.sum(~over))
        y[over] = y[over] - (s2[over] - VarThresh)
        return y - beta * np.sqrt(s2)

    return logp


def build_case(name):
    from tests._cases import synth_problem

    D, N, S, E, W, Ns, thin, meanfun, low_noise, tight, VarThresh, beta, seed = CASES[name]
    p = synth_problem(seed, D, N, 3, S, meanfun=meanfun, noisy=False)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(0.03)
    if low_noise:                                      # the hyper-sample S // 2 on the Lchol = false branch (tests/_quad_ref.py::mixed_gp)
        hyp[D + 1, S // 2] = math.log(3e-4)
        hyp[:D, S // 2] += math.log(0.25)
    gp = R.gplite_post(hyp, p["X"], p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    X = gp["X"]
    rng = np.random.default_rng(seed + 1900)
    if tight:                                          # a box barely wider than the walkers' spread: stepping out leaves it
        xm = X[int(np.argmax(gp["y"]))]
        LB, UB = xm - 0.15, xm + 0.15
        x0 = xm[None, None, :] + 0.1 * (2 * rng.random((E, W, D)) - 1)
    else:
        diam = np.max(X, axis=0) - np.min(X, axis=0)
        LB, UB = np.min(X, axis=0) - 0.5 * diam, np.max(X, axis=0) + 0.5 * diam
        best = X[np.argsort(-gp["y"], kind="stable")[: max(4, N // 4)]]
        x0 = best[rng.integers(0, best.shape[0], size=(E, W))] + 0.05 * rng.standard_normal((E, W, D))
        x0 = np.minimum(np.maximum(x0, LB), UB)
    H = W // 2
    Nm = -(-Ns // E)
    burnin = burnin_of(Ns)
    M = I.halfmoves_needed(Nm, H, thin, burnin)
    U = rng.random((SLOTS, H, E, M + 1))
    U = np.minimum(np.maximum(U, 2.0 ** -53), 1.0 - 2.0 ** -53)
    return {"name": name, "gp": gp, "x0": x0, "LB": LB, "UB": UB, "U": U, "D": D, "N": N, "S": S, "E": E, "W": W, "H": H, "Ns": Ns, "Nm": Nm,
            "thin": thin, "burnin": burnin, "M": M, "VarThresh": VarThresh, "beta": beta}


def interleave(Xt, Ns):
    """Xt (Nm x D x E) -> X (Ns x D): row e + E i is record i of ensemble e"""
    Nm, D, E = Xt.shape
    return np.transpose(Xt, (0, 2, 1)).reshape(Nm * E, D)[:Ns].copy()


_RUNS = {}


def run_case(name):
    """the case and the restatement's answer, computed once per process and left unchanged: the dict of _issample_ref.sample (its Xa is
    Xt, Nm x D x E) with X, the interleaved rows, and the threshold's counts"""
    if name not in _RUNS:
        c = build_case(name)
        stats = {"active": 0, "inactive": 0}
        r = I.sample(log_gpfun(c["gp"], c["VarThresh"], c["beta"], stats), c["x0"], c["LB"], c["UB"], c["Nm"], c["U"], thin=c["thin"], burnin=c["burnin"])
        r["X"] = interleave(r["Xa"], c["Ns"])
        r.update(stats)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[name] = (c, r)
    return _RUNS[name]


# ---------------------------------------------------------------------------------------------------------------- the noise estimate
def noise_estimate(xx, gl, X_rescaled, sn2new):
    """gpsample_vbmc.m:32-33, :38 given the draws xx (transformed space): (pos, sn2_avg, VarThresh, gap) -- pos the nearest row of
    X_rescaled per draw (first minimum), gap the smallest relative difference of a draw's two smallest distances"""
    a = np.asarray(xx, dtype=np.float64) / np.asarray(gl, dtype=np.float64)[None, :]
    b = np.asarray(X_rescaled, dtype=np.float64)
    d2 = np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :] - 2 * a @ b.T
    pos = np.argmin(d2, axis=1)
    two = np.sort(d2, axis=1)[:, :2]
    gap = float(np.min((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], np.finfo(np.float64).tiny)))
    sn2_avg = float(np.mean(np.asarray(sn2new, dtype=np.float64)[pos]))
    return pos, sn2_avg, max(1.0, sn2_avg), gap


# name: (case of tests/_vptools_ref.py, N of the GP): a logit and bounded variables; a rotation and a scale
VP_CASES = {"B": ("B", 37), "C": ("C", 33)}
VP_SEED = 20240611
NNN = 300


def build_vp_case(name):
    """A posterior of tests/_vptools_ref.py and a GP on its transformed space (S = 2, the training noise made up: sn2new is an input)"""
    from tests import _vptools_ref as T
    from tests._cases import synth_problem

    vname, N = VP_CASES[name]
    vp = T.make_case(vname)
    D = int(vp["D"])
    p = synth_problem(3, D, N, 3, 2, meanfun=4, noisy=False)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(0.03)
    gp = R.gplite_post(hyp, p["X"], p["y"], meanfun=4, noisefun=p["noisefun"], s2=p["s2"])
    X = gp["X"]
    rng = np.random.default_rng(77)
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    # a box that cuts into the posterior's draws (component means ~ N(0, 1)), so that the clip of the start acts
    LB, UB = np.full(D, -0.9), np.full(D, 0.9)
    return {"vp": vp, "gp": gp, "D": D, "N": N, "LB": LB, "UB": UB,
            "noise": {"gplengthscale": gl, "X_rescaled": X / gl[None, :], "sn2new": 0.3 + 1.5 * rng.random(N)}}

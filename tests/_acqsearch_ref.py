"""NumPy restatement of the device-resident acquisition search (vbmc_acq_search, include/vbmc_hip.h): the (mu/mu_w, lambda)-CMA-ES of
vbmc_amd/optimize.py::cmaes_batched -- same constants, hsig, rank-one and rank-mu updates, step-size adaptation, stopping rules and
history window -- with the ONE departure the device form makes: the sampling transform is the lower Cholesky factor A of C, refreshed
every generation, Y = A Z, and ps is updated with A^-1 yw by forward substitution (Krause, Arnold & Glasmachers 2016).  Candidates are
clamped into [LB, UB]; the clamped points are evaluated, ranked (not finite = +Inf, stable) and fed back as y = (x - xmean) / sigma.

``fun(X)`` takes the lam x D points of a generation and returns lam values; ``acq_fun(...)`` builds one from the oracle's
acqwrapper_vbmc.  ``Z`` is D x lam x Gmax, generation g's normals Z[:, :, g]; running out of them raises, as the device call refuses.
The trace holds, per generation: the rank order, the sorted values, xmean and sigma after the update, C after the update, the factor A
and the points X that were evaluated."""
import math

import numpy as np

from oracle import vbmc_ref as R

STOPS = ("TolX", "TolFun", "TolHistFun", "MaxFunEvals", "MaxIter")


def default_popsize(D):
    return 4 + int(math.floor(3 * math.log(D)))


def constants(D, lam):
    mu = lam // 2
    wts = math.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    wts = wts / np.sum(wts)
    mueff = 1.0 / np.sum(wts ** 2)
    N = float(D)
    c = {"mu": mu, "wts": wts, "mueff": mueff}
    c["cc"] = (4 + mueff / N) / (N + 4 + 2 * mueff / N)
    c["cs"] = (mueff + 2) / (N + mueff + 5)
    c["c1"] = 2 / ((N + 1.3) ** 2 + mueff)
    c["cmu"] = min(1 - c["c1"], 2 * (mueff - 2 + 1 / mueff) / ((N + 2) ** 2 + mueff))
    c["damps"] = 1 + 2 * max(0.0, math.sqrt((mueff - 1) / (N + 1)) - 1) + c["cs"]
    c["chiN"] = math.sqrt(N) * (1 - 1 / (4 * N) + 1 / (21 * N * N))
    c["nh"] = 10 + int(math.ceil(30 * N / lam))
    return c


def chol_lower(C):
    """Column-by-column lower Cholesky factor; None when a pivot is not positive (or not a number)."""
    D = C.shape[0]
    A = np.zeros((D, D))
    for j in range(D):
        s = C[j, j] - np.dot(A[j, :j], A[j, :j])
        if not (s > 0.0) or not np.isfinite(s):
            return None
        A[j, j] = math.sqrt(s)
        if j + 1 < D:
            A[j + 1:, j] = (C[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    return A


def forward_subst(A, b):
    D = b.size
    v = np.zeros(D)
    r = b.astype(np.float64).copy()
    for i in range(D):
        v[i] = r[i] / A[i, i]
        r[i + 1:] -= A[i + 1:, i] * v[i]
    return v


def cmaes_chol(fun, x0, insigma, LB, UB, **kw):
    with np.errstate(all="ignore"):          # the indefinite-covariance cases overflow on purpose
        return _cmaes_chol(fun, x0, insigma, LB, UB, **kw)


def _cmaes_chol(fun, x0, insigma, LB, UB, *, TolX, TolFun, TolHistFun, MaxFunEvals=0, MaxIter=0, popsize=0, Z):
    xmean = np.asarray(x0, dtype=np.float64).reshape(-1).copy()
    D = xmean.size
    LB = np.asarray(LB, dtype=np.float64).reshape(D)
    UB = np.asarray(UB, dtype=np.float64).reshape(D)
    insigma = np.broadcast_to(np.asarray(insigma, dtype=np.float64).reshape(-1), (D,)).copy()
    lam = int(popsize) if popsize else default_popsize(D)
    c = constants(D, lam)
    mu, wts, mueff, cc, cs, c1, cmu, damps, chiN, nh = (c[k] for k in ("mu", "wts", "mueff", "cc", "cs", "c1", "cmu", "damps", "chiN", "nh"))
    sigma = float(np.max(insigma))
    C = np.diag((insigma / sigma) ** 2)
    pc, ps = np.zeros(D), np.zeros(D)
    MaxIter = int(MaxIter) if MaxIter else int(1e3 * (D + 5) ** 2 / math.sqrt(lam))
    hist = []
    evals, gen = 0, 0
    best_x, best_f = xmean.copy(), np.inf
    last_x, last_f = xmean.copy(), np.inf
    stop = "MaxIter"
    trace = []
    fixed = 0
    while gen < MaxIter:
        A = chol_lower(C)
        if A is None:                      # symmetric already: 1e-14 max diag onto the diagonal, once
            C = C.copy()
            C[np.arange(D), np.arange(D)] += 1e-14 * np.max(np.diag(C))
            A = chol_lower(C)
            fixed += 1
            if A is None:
                break
        if gen >= Z.shape[2]:
            raise ValueError("normal block exhausted")
        Zg = np.asarray(Z[:, :, gen], dtype=np.float64)
        X = np.minimum(np.maximum(xmean[:, None] + sigma * (A @ Zg), LB[:, None]), UB[:, None])
        Y = (X - xmean[:, None]) / sigma
        F = np.asarray(fun(np.ascontiguousarray(X.T)), dtype=np.float64).reshape(-1)
        gen += 1
        evals += lam
        F = np.where(np.isfinite(F), F, np.inf)
        order = np.argsort(F, kind="stable")
        last_f, last_x = float(F[order[0]]), X[:, order[0]].copy()
        if last_f < best_f:
            best_f, best_x = last_f, last_x.copy()
        ysel = Y[:, order[:mu]]
        yw = ysel @ wts
        xmean = xmean + sigma * yw
        ps = (1 - cs) * ps + math.sqrt(cs * (2 - cs) * mueff) * forward_subst(A, yw)
        nps = math.sqrt(float(np.sum(ps * ps)))
        hsig = float(nps / math.sqrt(1 - (1 - cs) ** (2 * gen)) / chiN < 1.4 + 2 / (D + 1))
        pc = (1 - cc) * pc + (hsig * math.sqrt(cc * (2 - cc) * mueff)) * yw
        dh = (1 - hsig) * cc * (2 - cc)
        C = (1 - c1 - cmu) * C + c1 * (np.outer(pc, pc) + dh * C) + cmu * ((ysel * wts[None, :]) @ ysel.T)
        C = np.tril(C) + np.tril(C, -1).T
        sigma = sigma * float(np.exp((cs / damps) * (nps / chiN - 1)))
        hist.append(last_f)
        trace.append({"order": order.copy(), "F": F[order].copy(), "xmean": xmean.copy(), "sigma": sigma, "C": C.copy(), "A": A, "X": X})
        sd = sigma * np.sqrt(np.maximum(np.diag(C), 0.0))
        win = hist[-min(nh, len(hist)):]
        with np.errstate(invalid="ignore"):
            if MaxFunEvals and MaxFunEvals > 0 and evals >= MaxFunEvals:
                stop = "MaxFunEvals"
                break
            if np.all(sd < TolX) and np.all(sigma * np.abs(pc) < TolX):
                stop = "TolX"
                break
            if gen > 2 and float(F[order[-1]]) - last_f < TolFun and (max(win) - min(win)) < TolFun:
                stop = "TolFun"
                break
            if len(hist) > nh and (max(hist[-nh:]) - min(hist[-nh:])) < TolHistFun:
                stop = "TolHistFun"
                break
    return {"xmin": last_x, "fmin": last_f, "xbest": best_x, "fbest": best_f, "xmean": xmean, "sigma": sigma, "C": C, "evals": evals,
            "generations": gen, "stop": stop, "trace": trace, "popsize": lam, "chol_fixed": fixed}


def acq_fun(vp, gp, optimState, name):
    """X (lam x D) -> acqwrapper_vbmc(X, vp, gp, optimState, 0, name) of the oracle."""
    return lambda X: np.asarray(R.acqwrapper_vbmc(X, vp, gp, optimState, name)[0], dtype=np.float64).reshape(-1)


def min_rank_gap(trace):
    """The smallest gap between neighbouring sorted values over a trace, relative to 1 + |F|: the trajectory comparison's guard."""
    worst = np.inf
    for t in trace:
        F = t["F"][np.isfinite(t["F"])]
        if F.size > 1:
            worst = min(worst, float(np.min(np.diff(F) / (1 + np.abs(F[:-1])))))
    return worst


def search_cases():
    """The cases of the GPU trajectory test (tests/test_gpu_acqsearch.py), by name: (D, N, S, K, acq, var_regularized, face, seed).
    ``face``: the start sits on a face of the box, so that clamping is active from the first generation.  The seeds are ones for which
    the restatement's own 20-generation trajectory keeps every gap between neighbouring sorted values above 1e-6 (1 + |F|)
    (tests/test_acqsearch_restatement.py asserts it): the density-weighted functions are of order 0.1 at low D and the log-valued one
    carries the cases at D = 10 and 32, where the others' values are far below that yardstick."""
    return {
        "D2": (2, 17, 1, 1, "acqf", True, False, 23),
        "D3": (3, 40, 3, 2, "acqus", True, False, 16),
        "D10": (10, 40, 3, 2, "acqflog", False, False, 2),
        "D32": (32, 40, 1, 2, "acqflog", True, False, 4),
        "face": (3, 17, 3, 1, "acqf", True, True, 33),
        "sn2": (4, 40, 3, 2, "acqfsn2", False, False, 3),
        "slab": (4, 1264, 1, 2, "acqflog", True, False, 42),       # N > 1248: the prediction's slab form
    }


def build_case(name):
    from tests import _quad_ref as Q

    D, N, S, K, acq, reg, face, seed = search_cases()[name]
    gp, p = Q.mixed_gp(seed, D, N, S, 4)
    rng = np.random.default_rng(seed + 50)
    X = gp["X"]
    mu = X[rng.permutation(N)[:K]].T.copy()
    sigma = 0.5 + 0.3 * rng.random(K)
    lam = 0.8 + 0.4 * rng.random(D)
    lam = lam * np.sqrt(D / np.sum(lam ** 2))
    w = rng.dirichlet(np.ones(K))
    vp = R.make_vp(mu, sigma, lam, eta=np.log(w))
    vp["w"] = w
    st = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": reg, "TolGPVar": 1e-4}
    if acq == "acqfsn2":
        gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
        gp = dict(gp, X_rescaled=X / gl[None, :], sn2new=0.01 + 0.1 * rng.random(N))
        st["gplengthscale"] = gl
    xr = np.max(X, axis=0) - np.min(X, axis=0)
    LB, UB = np.min(X, axis=0) - 0.1 * xr, np.max(X, axis=0) + 0.1 * xr
    x0 = X[int(np.argmax(gp["y"]))] + 0.05 * rng.standard_normal(D)
    x0 = np.minimum(np.maximum(x0, LB), UB)
    if face:
        x0[0] = UB[0]
        x0[-1] = LB[-1]
    insigma = 0.3 * np.std(X, axis=0)
    lamp = default_popsize(D)
    Z = rng.standard_normal((D, lamp, 24))
    return {"gp": gp, "vp": vp, "st": st, "acq": acq, "x0": x0, "insigma": insigma, "LB": LB, "UB": UB, "Z": Z, "D": D, "lam": lamp}


def run_case(case, gens=20):
    return cmaes_chol(acq_fun(case["vp"], case["gp"], case["st"], case["acq"]), case["x0"], case["insigma"], case["LB"], case["UB"],
                      TolX=0.0, TolFun=0.0, TolHistFun=0.0, MaxIter=gens, Z=case["Z"])


def repair_case(kind):
    """Two cases for the covariance repair, built on case D2.  "shift": insigma = (0.3, 1e-170), so the initial C = diag(1, 0) -- the
    square underflows -- is singular, the 1e-14 max diag shift makes it positive definite and the search goes on.  "indefinite": insigma
    1e-300 and normals of 1e300, so the first update overflows C to Inf, the shift cannot help and the search stops after one
    generation with MaxIter's code and the state so far.  (sigma Z is of order one there: the points are distinct and inside the box.)"""
    c = dict(build_case("D2"))
    z = np.random.default_rng(105).standard_normal(c["Z"].shape)     # a draw whose six generations keep the rank gap (asserted on the CPU)
    if kind == "shift":
        c["insigma"], c["Z"] = np.array([0.3, 1e-170]), z
    else:
        c["insigma"], c["Z"] = np.full(2, 1e-300), z * 1e300
    return c

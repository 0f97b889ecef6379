"""NumPy restatement of the mode search of vbmc_vp_mode (include/vbmc_hip.h), for tests/test_mode_restatement.py and
tests/test_gpu_mode.py.  File:line cites are relative to the reference tree.  Nothing here imports the package.

    objective(vp, u, origflag)   g(u) = log q(u) - logprob(u) (origflag) or log q(u), its gradient and Hessian.  log q is the mixture
                                 of vbmc_pdf.m:52-60 in the log domain (max-shifted, no underflow rule); logprob is
                                 warpvars_vbmc(u, 'logprob', trinfo) (vbmc_pdf.m:115, warpvars_vbmc.m:463-503, :762-767)
    rank_starts(vp, nmax, ...)   vbmc_mode.m:23-28: a stable ascending sort of -g at the K means, the first nmax (all K in index
                                 order for nmax >= K); with origflag ranked by g at the starts themselves
    bfgs(vp, u0, comp, ...)      the library's optimiser: H0 = diag((sigma_c lambda)^2), d = -H grad F for F = -g, candidates
                                 u + 2^-k d, k = 0 .. 31, the first with F(u + t d) <= F(u) + 1e-4 t grad F'd; the update skipped unless
                                 y's > 1e-10 |y| |s|; stops GRAD / STEP / MAXITER
    polish(vp, u, origflag)      Newton on the gradient with the analytic Hessian
    mode(vp, nmax, origflag)     all of it with the winner rule: the largest fs, the first of equal ones
"""
import numpy as np

from tests import _vptools_ref as V

STOP_GRAD, STOP_STEP, STOP_MAXITER = 1, 2, 3
KMAX, C1, CURV, W = 32, 1e-4, 1e-10, 4
TOL_GRAD, MAX_ITER = 1e-6, 200


def _parts(vp):
    D, K = int(vp["D"]), int(vp["K"])
    mu = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K).T
    return D, K, mu, np.ravel(vp["sigma"]).astype(float), np.ravel(vp["lambda"]).astype(float), np.ravel(vp["w"]).astype(float)


def _transform(vp):
    """(types, mu, delta, M) with v = M u the coordinate before rotation and scale (v = (u .* scale) R'), or None"""
    tr = vp.get("trinfo")
    if not tr:
        return None
    D = int(vp["D"])
    typ = np.asarray(tr["type"]).astype(int).ravel()
    scale = tr.get("scale")
    scale = np.ones(D) if scale is None or not np.any(np.asarray(scale) != 1) else np.asarray(scale, dtype=np.float64).ravel()
    R = tr.get("R_mat")
    R = np.eye(D) if R is None or np.size(R) == 0 else np.asarray(R, dtype=np.float64)
    return typ, np.ravel(tr["mu"]).astype(float), np.ravel(tr["delta"]).astype(float), R * scale[None, :]


def logq(vp, u, order=0):
    """log q(u) of the Gaussian mixture and, for order >= 1 / 2, its gradient / Hessian"""
    D, K, mu, sigma, lam, w = _parts(vp)
    u = np.asarray(u, dtype=np.float64).ravel()
    prec = 1.0 / (sigma[:, None] * lam[None, :]) ** 2                                 # K x D
    with np.errstate(divide="ignore"):
        a = np.log(w) - D * np.log(sigma) - 0.5 * np.sum((u - mu) ** 2 * prec, axis=1)
    m = np.max(a)
    e = np.exp(a - m)
    val = m + np.log(np.sum(e)) - 0.5 * D * np.log(2 * np.pi) - np.sum(np.log(lam))
    if order == 0:
        return val
    r = e / np.sum(e)
    gk = -(u - mu) * prec                                                             # K x D: the gradient of component k's exponent
    grad = r @ gk
    if order == 1:
        return val, grad
    H = -np.diag(r @ prec) + (gk * r[:, None]).T @ gk - np.outer(grad, grad)
    return val, grad, H


def logprob(vp, u, order=0):
    """warpvars_vbmc(u, 'logprob', trinfo) and its gradient / Hessian: d/dv_d = 0 (type 0), 1 (types 1, 2), -delta tanh(z / 2) with
    z = v delta + mu (type 3); then the chain rule through v = M u"""
    D = int(vp["D"])
    t = _transform(vp)
    u = np.asarray(u, dtype=np.float64).ravel()
    if t is None:
        return (0.0, np.zeros(D), np.zeros((D, D)))[: order + 1] if order else 0.0
    typ, tmu, tdel, M = t
    val = float(V.warp(u[None, :], "l", vp["trinfo"])[0])
    if order == 0:
        return val
    v = M @ u
    z = v * tdel + tmu
    dv = np.where(typ == 3, -tdel * np.tanh(z / 2), np.where((typ == 1) | (typ == 2), 1.0, 0.0))
    grad = M.T @ dv
    if order == 1:
        return val, grad
    hv = np.where(typ == 3, -0.5 * tdel ** 2 / np.cosh(z / 2) ** 2, 0.0)
    return val, grad, M.T @ (hv[:, None] * M)


def objective(vp, u, origflag, order=0):
    a = logq(vp, u, order)
    if not origflag:
        return a
    b = logprob(vp, u, order)
    return a - b if order == 0 else tuple(x - y for x, y in zip(a, b))


def rank_starts(vp, nmax, origflag):
    """(components of the starts in order, the objective at all K means)"""
    D, K, mu, *_ = _parts(vp)
    nmax = 20 if nmax is None or nmax <= 0 else int(nmax)
    f = np.array([objective(vp, mu[k], origflag) for k in range(K)])
    if nmax >= K:
        return np.arange(K), f
    return np.argsort(-f, kind="stable")[:nmax], f


def bfgs(vp, u0, comp, origflag, tol_grad=TOL_GRAD, max_iter=MAX_ITER):
    D, K, mu, sigma, lam, w = _parts(vp)
    u = np.array(u0, dtype=np.float64)
    H = np.diag((sigma[comp] * lam) ** 2)
    val, grad = objective(vp, u, origflag, 1)
    f, g = -val, -grad
    f0, it, nfev = f, 0, 1
    while True:
        if np.max(np.abs(g)) <= tol_grad:
            stop = STOP_GRAD
            break
        if it >= max_iter:
            stop = STOP_MAXITER
            break
        d = -H @ g
        gd = g @ d
        take = None
        for k in range(KMAX):
            if k % W == 0:
                nfev += W
            t = 2.0 ** -k
            val, grad = objective(vp, u + t * d, origflag, 1)
            if -val <= f + C1 * t * gd:
                take = (u + t * d, -val, -grad)
                break
        if take is None:
            stop = STOP_STEP
            break
        s, y = take[0] - u, take[2] - g
        ys, Hy = y @ s, H @ y
        if ys > 0 and ys * ys > CURV ** 2 * (s @ s) * (y @ y):
            rho = 1.0 / ys
            H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + rho * (1 + rho * (y @ Hy)) * np.outer(s, s)
        u, f, g = take
        it += 1
    return dict(u=u, f=-f, f0=-f0, iters=it, nfev=nfev, stop=stop)


def polish(vp, u, origflag, steps=20):
    """Newton on grad g = 0 from u; returns (u*, H(u*))"""
    u = np.array(u, dtype=np.float64)
    for _ in range(steps):
        _, g, H = objective(vp, u, origflag, 2)
        du = np.linalg.solve(H, g)
        u = u - du
        if np.max(np.abs(du)) <= 1e-15 * max(1.0, np.max(np.abs(u))):
            break
    return u, objective(vp, u, origflag, 2)[2]


def distance_bound(H, tol_grad=TOL_GRAD):
    """Two points with |grad g| <= tol_grad near one maximum with Hessian H are within 2 tol_grad |H^-1|_2 of each other, to first
    order: each is within |H^-1|_2 |grad g| of the maximum"""
    return 2.0 * tol_grad * np.linalg.norm(np.linalg.inv(H), 2)


def back(vp, u, origflag):
    """xs: u itself, or with origflag its inverse transform with the clamp [lb + eps(lb), ub - eps(ub)]"""
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    return V.warp(u, "i", vp.get("trinfo")) if origflag and vp.get("trinfo") else u.copy()


def winner(fs):
    """the largest fs, the first of equal ones (MATLAB's min of -fs)"""
    return int(np.argmax(np.asarray(fs)))


def mode(vp, nmax=20, origflag=True, tol_grad=TOL_GRAD, max_iter=MAX_ITER):
    D, K, mu, *_ = _parts(vp)
    comps, _ = rank_starts(vp, nmax, origflag)
    runs = [bfgs(vp, mu[c], c, origflag, tol_grad, max_iter) for c in comps]
    us = np.array([r["u"] for r in runs])
    fs = np.array([r["f"] for r in runs])
    idx = winner(fs)
    xs = back(vp, us, origflag)
    return dict(x=xs[idx], fval=fs[idx], idx=idx, start_comp=np.asarray(comps), us=us, xs=xs, fs=fs, f0=np.array([r["f0"] for r in runs]),
                iters=np.array([r["iters"] for r in runs]), nfev=np.array([r["nfev"] for r in runs]), stop=np.array([r["stop"] for r in runs]))


# ---------------------------------------------------------------------------------------------------------------- the test cases
def MIXED(D):
    """all four transform types in turn"""
    return [d % 4 for d in range(D)]


CASES = {   # name: (D, K, transform types or None, scale + rotation, nmax): every padded width and its padding, the lane seams of K,
            # several components per lane, both limits, both sides of nmax < K, no transform, each type alone, all four mixed
    "d1k1": (1, 1, None, False, 20),
    "d4k2_t0": (4, 2, [0] * 4, False, 1),
    "d5k63_t1": (5, 63, [1] * 5, False, 5),
    "d13k64_t2": (13, 64, [2] * 13, False, 20),
    "d17k65_t3": (17, 65, [3] * 17, False, 20),
    "d25k130_mix": (25, 130, MIXED(25), True, 5),
    "d32k512_mix": (32, 512, MIXED(32), True, 20),
    "d4k65_all": (4, 65, MIXED(4), True, 65),
    "d5k130_all": (5, 130, MIXED(5), True, 200),
    "d32k512_none": (32, 512, None, False, 1),
}


def make_case(name, seed=3):
    D, K, types, rot, nmax = CASES[name]
    return V.make_vp(D, K, types, rot, seed), nmax


def make_zero_weight():
    """D = 5, K = 4 with the transform of V.CASES['G']; component 1 has no weight and is among the starts"""
    return V.make_zero_weight((1,))


def make_isolated():
    """D = 4, K = 5, all four transform types: component 4 lies 40 sigma lambda from every other in each coordinate (its density
    at the others, and theirs at it, underflow)"""
    vp = V.make_vp(4, 5, [0, 1, 2, 3], False, 5)
    mu = np.array(vp["mu"])
    s = float(np.max(vp["sigma"]))
    mu[:, 4] = np.max(mu[:, :4], axis=1) + 40.0 * s * np.ravel(vp["lambda"])
    vp["mu"] = mu
    return vp


def make_duplicate():
    """D = 4, K = 6 with a rotation: components 2 and 5 are identical (mean, width and weight), so their ranked values are bit-equal"""
    vp = V.make_vp(4, 6, [3, 0, 1, 2], True, 7)
    mu, sigma, w = np.array(vp["mu"]), np.array(vp["sigma"]), np.array(vp["w"])
    mu[:, 5], sigma[5], w[5] = mu[:, 2], sigma[2], w[2]
    vp.update(mu=mu, sigma=sigma, w=w / w.sum())
    return vp


def make_merged_pair(D=3, a=0.2):
    """Two equal components at +-a e_1 with a < sigma lambda_1: log q has its single mode at the midpoint, the origin"""
    lam = np.array([1.0, 0.8, 1.25])[:D]
    mu = np.zeros((D, 2))
    mu[0] = [a, -a]
    vp = dict(D=D, K=2, mu=mu, sigma=np.array([0.5, 0.5]), w=np.array([0.5, 0.5]), trinfo=None)
    vp["lambda"] = lam
    assert a < 0.5 * lam[0]
    return vp

"""Generate tests/golden/mp_quad_case*.json: 50-digit mpmath evaluation of gplite_quad from its definition.

TEST INFRASTRUCTURE.  An independent scalar-loop evaluation (no NumPy broadcasting, no code shared with tests/_quad_ref.py or
oracle/) of the Bayesian-quadrature integral of a GP with SE-ARD covariance against N(mu_i, diag sigma^2)
(gplite/gplite_quad.m:1-119), per hyper-sample s:

  z_n   = sf2 prod_d ell_d / tau_d  exp(-1/2 sum_d (mu_d - X_nd)^2 / tau_d^2),  tau_d^2 = sigma_d^2 + ell_d^2
          (the integral of k(x, X_n) N(x; mu, diag sigma^2) dx in closed form)
  F     = sum_n z_n alpha_n + the integral of the mean function,  alpha = (K + sn2 I)^-1 (y - m(X))
          mean 0: 0;  mean 1: m0;  mean 4: m0 - 1/2 sum_d ((mu_d - xm_d)^2 + sigma_d^2) / omega_d^2
  varF  = max(eps, sf2 prod_d ell_d / sqrt(2 sigma_d^2 + ell_d^2) - z' (K + sn2 I)^-1 z)

with (K + sn2 I)^-1 applied through mpmath's own LU solve.  The factors the library is handed (gp.post(s).alpha and L: the upper
Cholesky factor of K / sn2 + I, or -inv(K + sn2 I) when sn2 < 1e-6, gplite_core.m:67-99) are stored at 50-digit accuracy too, so
that a test can plug them in and measure the quadrature alone.

Run:  python tools/mp_quad_golden.py   (writes tests/golden/mp_quad_case{1,2,3}.json; the inputs are drawn with numpy
default_rng(seed) and stored next to the expected outputs, so the fixtures are self-contained data).
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = mp.mpf(2) ** -52


def M(x):
    return mp.mpf(float(x))


def chol_upper(A):
    n = len(A)
    R = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        R[j][j] = mp.sqrt(A[j][j] - mp.fsum(R[i][j] ** 2 for i in range(j)))
        for c in range(j + 1, n):
            R[j][c] = (A[j][c] - mp.fsum(R[i][j] * R[i][c] for i in range(j))) / R[j][j]
    return R


def quad_sample(hyp, X, y, meanfun, mu, sigma):
    """One hyper-sample -> dict(alpha, L, Lchol, F[i], varF[i], nf_kk)."""
    N, D = len(X), len(X[0])
    ell = [mp.e ** hyp[d] for d in range(D)]
    sf2 = mp.e ** (2 * hyp[D])
    sn2 = mp.e ** (2 * hyp[D + 1])
    hm = hyp[D + 2:]
    m0 = hm[0] if meanfun > 0 else mp.mpf(0)

    def mean_at(x):
        if meanfun != 4:
            return m0
        return m0 - mp.fsum(((x[d] - hm[1 + d]) / mp.e ** hm[D + 1 + d]) ** 2 for d in range(D)) / 2

    Kn = mp.matrix(N, N)
    for a in range(N):
        for b in range(N):
            Kn[a, b] = sf2 * mp.e ** (-mp.fsum(((X[a][d] - X[b][d]) / ell[d]) ** 2 for d in range(D)) / 2) + (sn2 if a == b else 0)
    r = mp.matrix([y[n] - mean_at(X[n]) for n in range(N)])
    alpha = mp.lu_solve(Kn, r)
    lchol = sn2 >= mp.mpf("1e-6")
    if lchol:
        L = chol_upper([[(Kn[a, b] - (sn2 if a == b else 0)) / sn2 + (1 if a == b else 0) for b in range(N)] for a in range(N)])
    else:
        Ki = Kn ** -1
        L = [[-Ki[a, b] for b in range(N)] for a in range(N)]
    nf_kk = sf2 * mp.fprod(ell[d] / mp.sqrt(2 * sigma[d] ** 2 + ell[d] ** 2) for d in range(D))
    F, varF = [], []
    for m in mu:
        z = mp.matrix([sf2 * mp.fprod(ell[d] / mp.sqrt(sigma[d] ** 2 + ell[d] ** 2) for d in range(D))
                       * mp.e ** (-mp.fsum((m[d] - X[n][d]) ** 2 / (sigma[d] ** 2 + ell[d] ** 2) for d in range(D)) / 2) for n in range(N)])
        f = mp.fsum(z[n] * alpha[n] for n in range(N)) + m0
        if meanfun == 4:
            f -= mp.fsum(((m[d] - hm[1 + d]) ** 2 + sigma[d] ** 2) / (mp.e ** hm[D + 1 + d]) ** 2 for d in range(D)) / 2
        Kiz = mp.lu_solve(Kn, z)
        F.append(f)
        varF.append(max(EPS, nf_kk - mp.fsum(z[n] * Kiz[n] for n in range(N))))
    return {"alpha": [alpha[n] for n in range(N)], "L": L, "Lchol": bool(lchol), "F": F, "varF": varF, "nf_kk": nf_kk}


def make_case(seed, D, N, S, Nstar, meanfun, sigma, logsn):
    rng = np.random.default_rng(seed)
    X = 1.5 * rng.standard_normal((N, D))
    y = -0.5 * np.sum(X ** 2, axis=1) + 0.3 * rng.standard_normal(N)
    nmean = {0: 0, 1: 1, 4: 2 * D + 1}[meanfun]
    hyp = np.zeros((D + 2 + nmean, S))
    for s in range(S):
        hyp[:D, s] = np.log(0.7) + 0.2 * rng.standard_normal(D)
        hyp[D, s] = np.log(1.3) + 0.1 * rng.standard_normal()
        hyp[D + 1, s] = logsn[s]
        if meanfun >= 1:
            hyp[D + 2, s] = 0.4 + 0.1 * rng.standard_normal()
        if meanfun == 4:
            hyp[D + 3:D + 3 + D, s] = 0.2 * rng.standard_normal(D)
            hyp[D + 3 + D:, s] = np.log(2.0) + 0.1 * rng.standard_normal(D)
    mu = np.vstack([1.2 * rng.standard_normal((Nstar - 1, D)), X[:1] + 0.01])     # the last point beside a training input
    return {"D": D, "N": N, "S": S, "Nstar": Nstar, "meanfun": meanfun, "X": X, "y": y, "hyp": hyp, "mu": mu,
            "sigma": np.asarray(sigma, dtype=np.float64)}


def fl(v):
    if isinstance(v, (list, tuple)):
        return [fl(t) for t in v]
    return float(v)


def run_case(c):
    X = [[M(v) for v in row] for row in c["X"]]
    y = [M(v) for v in c["y"]]
    mu = [[M(v) for v in row] for row in c["mu"]]
    sigma = [M(v) for v in c["sigma"]]
    S = c["S"]
    res = [quad_sample([M(v) for v in c["hyp"][:, s]], X, y, c["meanfun"], mu, sigma) for s in range(S)]
    exp = {k: fl([r[k] for r in res]) for k in ("alpha", "L", "F", "varF", "nf_kk")}     # S x ...
    exp["Lchol"] = [r["Lchol"] for r in res]
    # averaged over the hyper-samples (gplite_quad.m:112-119)
    if S > 1:
        Fbar = [mp.fsum(r["F"][i] for r in res) / S for i in range(c["Nstar"])]
        vss = [mp.fsum((r["F"][i] - Fbar[i]) ** 2 for r in res) / (S - 1) for i in range(c["Nstar"])]
        exp["F_avg"] = fl(Fbar)
        exp["varF_avg"] = fl([mp.fsum(r["varF"][i] for r in res) / S + vss[i] for i in range(c["Nstar"])])
    inputs = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return {"inputs": inputs, "expected": exp}


CASES = [
    # seed, D, N, S, Nstar, meanfun, sigma, log sn per hyper-sample
    (101, 1, 6, 2, 3, 0, [0.3], [np.log(0.05), np.log(0.1)]),
    (102, 3, 12, 3, 5, 4, [0.2, 0.0, 0.5], [np.log(0.05), np.log(3e-4), np.log(0.02)]),     # a zero sigma entry; sn2 = 9e-8 < 1e-6
    (103, 2, 9, 2, 4, 1, [0.1, 0.4], [np.log(0.03), np.log(0.2)]),
]


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    for i, args in enumerate(CASES, 1):
        with open(os.path.join(out, "mp_quad_case%d.json" % i), "w") as f:
            json.dump(run_case(make_case(*args)), f)
        print("wrote mp_quad_case%d.json" % i)


if __name__ == "__main__":
    main()

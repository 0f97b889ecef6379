"""Writes tests/golden/mp_mode_case{0..4}.json: the objective of vbmc_vp_mode -- log q(u) for origflag = 0 and
g(u) = log q(u) - logprob(u) for origflag = 1, logprob the log-Jacobian of shared/warpvars_vbmc.m:463-503, :762-767 -- evaluated with
mpmath at 50 digits on tiny shapes (D <= 3, K <= 4; each transform type, scale and rotation), its gradient, and the maximiser reached
from each component mean.  tests/test_mode_restatement.py holds the NumPy restatement tests/_mode_ref.py to these values.

The value is formed from the definitions (the sum of the component densities, its logarithm, the log-Jacobian term by term); the
gradient is mpmath's numerical derivative of that value at 50 digits, not a second copy of the analytic formula; a maximiser is
mpmath's findroot on that gradient, started from the float64 answer of the restatement's optimiser.

    python tools/gen_mode_golden.py
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp.mp.dps = 50
CASES = [   # D, K, types, scale + rotation, seed
    dict(D=1, K=2, types=None, rot=False, seed=21),
    dict(D=2, K=3, types=[0, 1], rot=False, seed=22),
    dict(D=2, K=3, types=[2, 3], rot=False, seed=23),
    dict(D=3, K=4, types=[3, 0, 1], rot=True, seed=24),
    dict(D=3, K=2, types=[1, 2, 3], rot=True, seed=25),
]
NPOINTS = 4


def logq(u, vp):
    D, K = vp["D"], vp["K"]
    lam = [mp.mpf(float(v)) for v in vp["lambda"]]
    tot = mp.mpf(0)
    for k in range(K):
        sg, w = mp.mpf(float(vp["sigma"][k])), mp.mpf(float(vp["w"][k]))
        d2 = sum(((u[d] - mp.mpf(float(vp["mu"][d][k]))) / (sg * lam[d])) ** 2 for d in range(D))
        tot += w / sg ** D * mp.exp(-d2 / 2)                                                       # vbmc_pdf.m:59-60
    nf = 1 / (2 * mp.pi) ** (mp.mpf(D) / 2) / mp.fprod(lam)                                        # :56
    return mp.log(nf * tot)


def logprob(u, vp):
    tr = vp["trinfo"]
    if tr is None:
        return mp.mpf(0)
    D = vp["D"]
    y = [u[d] * (mp.mpf(float(tr["scale"][d])) if tr["scale"] is not None else 1) for d in range(D)]            # warpvars_vbmc.m:466
    if tr["R_mat"] is not None:
        y = [sum(y[j] * mp.mpf(float(tr["R_mat"][i][j])) for j in range(D)) for i in range(D)]                   # :469  y R'
    p = mp.mpf(0)
    for d in range(D):
        t = int(tr["type"][d])
        a, b, m, dl = (mp.mpf(float(tr[n][d])) if np.isfinite(tr[n][d]) else None for n in ("lb_orig", "ub_orig", "mu", "delta"))
        if t == 0:
            p += mp.log(dl)                                                                                      # :487
        elif t in (1, 2):
            p += y[d]                                                                                            # :493
        else:
            z = y[d] * dl + m
            p += mp.log(b - a) + (-z - 2 * mp.log(1 + mp.exp(-z))) + mp.log(dl)                                  # :499-502
    if tr["scale"] is not None:
        p += sum(mp.log(mp.mpf(float(s))) for s in tr["scale"])                                                  # :764
    return p


def objective(u, vp, origflag):
    return logq(u, vp) - (logprob(u, vp) if origflag else 0)


def gradient(u, vp, origflag):
    D = vp["D"]
    return [mp.diff(lambda *x: objective(list(x), vp, origflag), tuple(u), tuple(1 if e == d else 0 for e in range(D))) for d in range(D)]


def lists(vp):
    out = {k: (np.asarray(v).tolist() if v is not None else None) for k, v in vp.items() if k != "trinfo"}
    tr = vp["trinfo"]
    out["trinfo"] = None if tr is None else {k: (None if v is None else [None if not np.isfinite(x) else x for x in np.ravel(v).tolist()] if k in ("lb_orig", "ub_orig")
                                                 else np.asarray(v).tolist()) for k, v in tr.items()}
    return out


def main():
    from tests import _mode_ref as R
    from tests import _vptools_ref as T

    for i, c in enumerate(CASES):
        vp = T.make_vp(c["D"], c["K"], c["types"], c["rot"], c["seed"], width=1.5)
        D, K = c["D"], c["K"]
        rng = np.random.default_rng(100 + i)
        pts = np.asarray(vp["mu"]).T[rng.integers(0, K, NPOINTS)] + 0.3 * rng.normal(size=(NPOINTS, D))
        rec = {"vp": lists(vp), "points": pts.tolist(), "flags": {}}
        for origflag in (0, 1):
            f = {"value": [], "gradient": [], "maximiser": [], "stop": []}
            for p in pts:
                u = [mp.mpf(float(v)) for v in p]
                f["value"].append(mp.nstr(objective(u, vp, origflag), 30))
                f["gradient"].append([mp.nstr(g, 30) for g in gradient(u, vp, origflag)])
            for k in range(K):
                r = R.bfgs(vp, np.asarray(vp["mu"])[:, k], k, origflag)
                root = mp.findroot(lambda *x: gradient(list(x), vp, origflag), tuple(mp.mpf(float(v)) for v in r["u"]), tol=mp.mpf(10) ** -35)
                f["maximiser"].append([mp.nstr(v, 30) for v in root])
                f["stop"].append(int(r["stop"]))
            rec["flags"][str(origflag)] = f
        path = os.path.join(ROOT, "tests", "golden", "mp_mode_case%d.json" % i)
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)
        print(path)


if __name__ == "__main__":
    main()

"""Writes tests/golden/mp_vptools_case{0..5}.json: the variable transform of shared/warpvars_vbmc.m (types 0-3, scale, rotation) and
vbmc_pdf.m's three density families evaluated with mpmath at 50 digits on tiny shapes (D <= 7, K <= 4, <= 8 points).  A generator
of its own beside oracle/mp_golden.py; tests/test_vptools_restatement.py holds the NumPy restatement to these values and
tests/test_gpu_vptools_edges.py the device.

And tests/golden/mp_vptools_band.json: two D = 2, K = 2 mixtures (the second with a logit transform of coordinate 2) at points on a
ray from the heavier component's mean along coordinate 1, placed so that the log of the transformed-space mixture takes chosen values
on both sides of log(realmin) and of log(5e-324), below which the device returns -Inf resp. 0.  No stored
value lies within 1e-6 of log(5e-324), so that the side a point is on is never a matter of rounding.

    python tools/gen_vptools_golden.py
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [   # D, K, types, scale + rotation, points, df of the t families (None: Gaussian only), gradient
    dict(D=1, K=1, types=None, rot=False, N=4, dfs=[], grad=True),
    dict(D=3, K=2, types=[0, 1, 2], rot=False, N=6, dfs=[], grad=True),
    dict(D=3, K=4, types=[3, 0, 3], rot=True, N=8, dfs=[], grad=False),
    dict(D=2, K=4, types=[3, 1], rot=False, N=8, dfs=[4.0, -3.0], grad=False),
    dict(D=7, K=3, types=[3, 0, 1, 2, 3, 0, 1], rot=True, N=6, dfs=[], grad=True),      # the padded width 8 with a rotation
    dict(D=6, K=4, types=None, rot=False, N=6, dfs=[4.0, -3.0], grad=True),
]
LOG_DENORM_MIN = -744.4400719213812    # VPT_LOG_DENORM_MIN (vbmc_amd/csrc/vp_tools_kernels.h)
BAND_TARGETS = [-690.0, -705.0, -708.3, -708.5, -720.0, -740.0, -744.3, -744.6, -745.2, -760.0, -1000.0, -1e5]
BAND_DFS = [5.0, -5.0]


def M(a):
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())


def direct(x, tr):
    D = len(x)
    u = []
    for d in range(D):
        t, a, b, m, dl = tr["type"][d], mp.mpf(tr["lb_orig"][d]), mp.mpf(tr["ub_orig"][d]), mp.mpf(tr["mu"][d]), mp.mpf(tr["delta"][d])
        if t == 0:
            u.append((x[d] - m) / dl)
        elif t == 1:
            u.append(mp.log(x[d] - a))
        elif t == 2:
            u.append(mp.log(b - x[d]))
        else:
            z = (x[d] - a) / (b - a)
            u.append((mp.log(z / (1 - z)) - m) / dl)
    if tr.get("R_mat") is not None:
        R = tr["R_mat"]
        u = [sum(u[i] * mp.mpf(R[i][j]) for i in range(D)) for j in range(D)]
    if tr.get("scale") is not None:
        u = [u[d] / mp.mpf(tr["scale"][d]) for d in range(D)]
    return u


def unrotate(y, tr):
    D = len(y)
    v = [y[d] * mp.mpf(tr["scale"][d]) for d in range(D)] if tr.get("scale") is not None else list(y)
    if tr.get("R_mat") is not None:
        R = tr["R_mat"]
        v = [sum(v[j] * mp.mpf(R[i][j]) for j in range(D)) for i in range(D)]
    return v


def inverse(y, tr):
    u = unrotate(y, tr)
    x = []
    for d in range(len(y)):
        t, a, b, m, dl = tr["type"][d], mp.mpf(tr["lb_orig"][d]), mp.mpf(tr["ub_orig"][d]), mp.mpf(tr["mu"][d]), mp.mpf(tr["delta"][d])
        if t == 0:
            x.append(u[d] * dl + m)
        elif t == 1:
            x.append(mp.exp(u[d]) + a)
        elif t == 2:
            x.append(b - mp.exp(u[d]))
        else:
            x.append(a + (b - a) / (1 + mp.exp(-(u[d] * dl + m))))
    return x


def logjac(y, tr):
    u = unrotate(y, tr)
    s = mp.mpf(0)
    for d in range(len(y)):
        t, a, b, m, dl = tr["type"][d], mp.mpf(tr["lb_orig"][d]), mp.mpf(tr["ub_orig"][d]), mp.mpf(tr["mu"][d]), mp.mpf(tr["delta"][d])
        if t == 0:
            s += mp.log(dl)
        elif t in (1, 2):
            s += u[d]
        else:
            z = u[d] * dl + m
            s += mp.log(b - a) - z - 2 * mp.log1p(mp.exp(-z)) + mp.log(dl)
        if tr.get("scale") is not None:
            s += mp.log(mp.mpf(tr["scale"][d]))
    return s


def density(vp, y, df):
    """(p, dp/dy) of the mixture at the transformed-space point y"""
    D, K = vp["D"], vp["K"]
    lam = [mp.mpf(v) for v in vp["lambda"]]
    p, g = mp.mpf(0), [mp.mpf(0)] * D
    for k in range(K):
        sg, w = mp.mpf(vp["sigma"][k]), mp.mpf(vp["w"][k])
        z = [(y[d] - mp.mpf(vp["mu"][d][k])) / (sg * lam[d]) for d in range(D)]
        d2 = sum(v * v for v in z)
        if df is None:
            n = w / sg ** D * mp.exp(-d2 / 2) / (2 * mp.pi) ** (mp.mpf(D) / 2) / mp.fprod(lam)
            g = [g[d] - n * (y[d] - mp.mpf(vp["mu"][d][k])) / (lam[d] ** 2 * sg ** 2) for d in range(D)]
        elif df > 0:
            nu = mp.mpf(df)
            n = w / sg ** D * mp.gamma((nu + D) / 2) / mp.gamma(nu / 2) / (nu * mp.pi) ** (mp.mpf(D) / 2) / mp.fprod(lam) * (1 + d2 / nu) ** (-(nu + D) / 2)
        else:
            nu = mp.mpf(-df)
            c = mp.gamma((nu + 1) / 2) / mp.gamma(nu / 2) / mp.sqrt(nu * mp.pi)
            n = w / sg ** D * c ** D / mp.fprod(lam) * mp.fprod([(1 + v * v / nu) ** (-(nu + 1) / 2) for v in z])
        p += n
    return p, g


def build(idx, c):
    r = np.random.default_rng(100 + idx)
    D, K, N = c["D"], c["K"], c["N"]
    vp = dict(D=D, K=K, mu=r.normal(0, 1, (D, K)).tolist(), sigma=np.exp(r.normal(-1, .3, K)).tolist(),
              w=r.dirichlet(np.ones(K)).tolist())
    vp["lambda"] = np.exp(r.normal(0, .3, D)).tolist()
    tr = None
    if c["types"] is not None:
        lb, ub = [-np.inf] * D, [np.inf] * D
        tmu, tdel = r.normal(0, .3, D).tolist(), np.exp(r.normal(0, .3, D)).tolist()
        for d, t in enumerate(c["types"]):
            if t in (1, 3):
                lb[d] = float(r.uniform(-2, 0))
            if t in (2, 3):
                ub[d] = float(r.uniform(1, 4))
            if t in (1, 2):
                tmu[d], tdel[d] = 0.0, 1.0
        tr = dict(lb_orig=lb, ub_orig=ub, type=list(c["types"]), mu=tmu, delta=tdel, scale=None, R_mat=None)
        if c["rot"]:
            tr["R_mat"] = np.linalg.qr(r.normal(size=(D, D)))[0].tolist()
            tr["scale"] = np.exp(r.normal(0, .2, D)).tolist()
    # points: transformed-space draws of the mixture, taken back to the original space in fp64 (the inputs are these doubles)
    comp = r.integers(0, K, N)
    Y = (np.asarray(vp["mu"])[:, comp].T + np.asarray(vp["lambda"]) * (r.normal(size=(N, D)) * np.asarray(vp["sigma"])[comp][:, None]))
    X = Y if tr is None else np.array([[float(v) for v in inverse([mp.mpf(t) for t in row], tr)] for row in Y])
    out = dict(vp=vp, trinfo=tr, X=X.tolist(), Y=Y.tolist(), dfs=c["dfs"], direct=[], inverse=[], logjac=[], logpdf_orig=[], logpdf_trans=[],
               pdf_orig=[], heavy={str(df): [] for df in c["dfs"]}, grad=[] if c["grad"] else None, gradlog=[] if c["grad"] else None)
    f = lambda v: float(mp.nstr(v, 20))
    for n in range(N):
        x = [mp.mpf(v) for v in X[n]]
        yt = [mp.mpf(v) for v in Y[n]]
        y = x if tr is None else direct(x, tr)
        lj = mp.mpf(0) if tr is None else logjac(y, tr)
        p, _ = density(vp, y, None)
        out["direct"].append([f(v) for v in y])
        out["inverse"].append([f(v) for v in (yt if tr is None else inverse(yt, tr))])
        out["logjac"].append(f(mp.mpf(0) if tr is None else logjac(yt, tr)))
        out["logpdf_orig"].append(f(mp.log(p) - lj))
        out["pdf_orig"].append(f(p / mp.exp(lj)))
        pt, gt = density(vp, yt, None)
        out["logpdf_trans"].append(f(mp.log(pt)))
        if c["grad"]:
            out["grad"].append([f(v) for v in gt])
            out["gradlog"].append([f(v / pt) for v in gt])
        for df in c["dfs"]:
            ph, _ = density(vp, y, df)
            out["heavy"][str(df)].append(f(mp.log(ph) - lj))
    return out


def build_band():
    f = lambda v: float(mp.nstr(v, 20))
    out = dict(threshold=LOG_DENORM_MIN, dfs=BAND_DFS, mixtures=[])
    for j in range(2):
        # the lighter component lies behind the ray's origin: the mixture decreases along the ray
        vp = dict(D=2, K=2, mu=[[0.4, -1.1], [-0.3, 0.6]], sigma=[0.35, 0.5], w=[0.7, 0.3])
        vp["lambda"] = [1.1, 0.8]
        tr = None
        if j == 1:
            tr = dict(lb_orig=[-np.inf, -1.0], ub_orig=[np.inf, 3.0], type=[0, 3], mu=[0.1, 0.2], delta=[0.9, 1.3], scale=None, R_mat=None)

        def point(t):
            """the original-space doubles of the ray's point at t, and what they are exactly in the transformed space"""
            y = [mp.mpf(vp["mu"][0][0]) + t, mp.mpf(vp["mu"][1][0]) + mp.mpf("0.05")]
            x = [float(v) for v in (y if tr is None else inverse(y, tr))]
            xm = [mp.mpf(v) for v in x]
            return x, (xm if tr is None else direct(xm, tr))

        def logmix(t):
            return mp.log(density(vp, point(t)[1], None)[0])

        ts = [mp.findroot(lambda t: logmix(t) - target, (mp.mpf(1), mp.mpf(200)), solver="anderson", tol=1e-20) for target in BAND_TARGETS]
        ts += [mp.mpf("0.3"), mp.mpf("-1.7")]                                  # two ordinary points
        m = dict(vp=vp, trinfo=tr, X=[], logmix_trans=[], logjac=[], logpdf_orig=[], pdf_orig=[], heavy={str(df): [] for df in BAND_DFS})
        for i, t in enumerate(ts):
            x, y = point(t)
            lm = mp.log(density(vp, y, None)[0])
            lj = mp.mpf(0) if tr is None else logjac(y, tr)
            if i < len(BAND_TARGETS):
                assert abs(lm - BAND_TARGETS[i]) <= 0.05, (j, i, lm)
            for v in (lm, lm - lj):
                assert abs(v - LOG_DENORM_MIN) > 1e-6, (j, i, v)
            m["X"].append(x)
            m["logmix_trans"].append(f(lm))
            m["logjac"].append(f(lj))
            m["logpdf_orig"].append(f(lm - lj))
            m["pdf_orig"].append(f(mp.exp(lm - lj)))
            for df in BAND_DFS:
                m["heavy"][str(df)].append(f(mp.log(density(vp, y, df)[0]) - lj))
        out["mixtures"].append(m)
    return out


if __name__ == "__main__":
    for i, c in enumerate(CASES):
        path = os.path.join(ROOT, "tests", "golden", "mp_vptools_case%d.json" % i)
        with open(path, "w") as fh:
            json.dump(build(i, c), fh, indent=1)
        print("wrote", path)
    path = os.path.join(ROOT, "tests", "golden", "mp_vptools_band.json")
    with open(path, "w") as fh:
        json.dump(build_band(), fh, indent=1)
    print("wrote", path)

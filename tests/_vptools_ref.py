"""NumPy restatement of the reference's variational-posterior tools, for the tests of vbmc_amd.vptools and of the vbmc_vp_* entry
points.  File:line cites are relative to the reference tree.  Nothing here imports the package.

    warp(x, action, tr)          shared/warpvars_vbmc.m: 'd' :77-111, :273-279; 'i' :282-320, :456-460; 'l' :463-503, :762-767
    pdf(vp, X, ...)              vbmc_pdf.m:28-124, the direct sum, all three density families, the gradient of :62-65, :108
    split / perm / rnd           vbmc_rnd.m:51-105 on the indexed block (sample i owns B[i]: a uniform, then D normals)
    moments(X)                   vbmc_moments.m:23-28
    kldiv(vp1, vp2, xx1, xx2)    vbmc_kldiv.m:70-88 given the two sets of draws
    mvnkl                        shared/mvnkl.m
"""
import numpy as np
from scipy.special import gammaln


# ---------------------------------------------------------------------------------------------------------------- the transform
def warp(x, action, tr):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    act = action[0]
    if not tr:                                                                       # :47-58
        return x.copy() if act in "di" else (np.zeros(len(x)) if act == "l" else np.ones(len(x)))
    typ = np.asarray(tr["type"]).astype(int).ravel()
    a, b, mu, delta = (np.asarray(tr[k], dtype=np.float64).ravel() for k in ("lb_orig", "ub_orig", "mu", "delta"))
    scale = tr.get("scale")
    scale = None if scale is None or not np.any(np.asarray(scale) != 1) else np.asarray(scale, dtype=np.float64).ravel()   # :66-69
    R = tr.get("R_mat")
    R = None if R is None or np.size(R) == 0 else np.asarray(R, dtype=np.float64)
    with np.errstate(all="ignore"):
        if act == "d":
            y = x.copy()
            for d, t in enumerate(typ):
                if t == 0:
                    y[:, d] = (x[:, d] - mu[d]) / delta[d]                           # :88
                elif t == 1:
                    y[:, d] = np.log(x[:, d] - a[d])                                 # :94
                elif t == 2:
                    y[:, d] = np.log(b[d] - x[:, d])                                 # :100
                elif t == 3:
                    z = (x[:, d] - a[d]) / (b[d] - a[d])                             # :106-109
                    y[:, d] = (np.log(z / (1 - z)) - mu[d]) / delta[d]
                else:
                    raise NotImplementedError(t)
            if R is not None:
                y = y @ R                                                            # :274
            if scale is not None:
                y = y / scale                                                        # :277
            return y
        y = x * scale if scale is not None else x.copy()                             # :285 / :466
        if R is not None:
            y = y @ R.T                                                              # :288 / :469
        if act == "i":
            out = y.copy()
            for d, t in enumerate(typ):
                if t == 0:
                    out[:, d] = y[:, d] * delta[d] + mu[d]                           # :299
                elif t == 1:
                    out[:, d] = np.exp(y[:, d]) + a[d]                               # :305
                elif t == 2:
                    out[:, d] = b[d] - np.exp(y[:, d])                               # :311
                elif t == 3:
                    z = y[:, d] * delta[d] + mu[d]                                   # :317-319
                    out[:, d] = a[d] + (b[d] - a[d]) * (1.0 / (1.0 + np.exp(-z)))
                else:
                    raise NotImplementedError(t)
            lo, hi = clamp_ends(tr)
            return np.minimum(np.maximum(out, lo), hi)                               # :459
        p = np.zeros_like(y)
        for d, t in enumerate(typ):
            if t == 0:
                p[:, d] = np.log(delta[d])                                           # :487
            elif t in (1, 2):
                p[:, d] = y[:, d]                                                    # :493
            elif t == 3:
                z = y[:, d] * delta[d] + mu[d]                                       # :499-502
                p[:, d] = np.log(b[d] - a[d]) + (-z + 2 * (-np.log1p(np.exp(-z)))) + np.log(delta[d])
            else:
                raise NotImplementedError(t)
        if scale is not None:
            p = p + np.log(scale)                                                    # :764
        p = p.sum(axis=1)                                                            # :767
        return p if act == "l" else np.exp(p)


def clamp_ends(tr):
    """:456-458: a + eps(a), b - eps(b) for the finite bounds"""
    a, b = (np.asarray(tr[k], dtype=np.float64).ravel() for k in ("lb_orig", "ub_orig"))
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isfinite(a), a + np.spacing(np.abs(a)), a)
        hi = np.where(np.isfinite(b), b - np.spacing(np.abs(b)), b)
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------- vbmc_pdf
def pdf(vp, X, origflag=True, logflag=False, transflag=False, df=np.inf, grad=False):
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    tr = vp.get("trinfo")
    if origflag and tr and not transflag:
        X = warp(X, "d", tr)                                                         # :36-39
    N, D = X.shape
    K = int(vp["K"])
    w, lam, sigma = np.ravel(vp["w"]), np.ravel(vp["lambda"]), np.ravel(vp["sigma"])
    mu_t = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K).T
    y = np.zeros(N)
    dy = np.zeros((N, D))
    with np.errstate(all="ignore"):
        if not np.isfinite(df) or df == 0:
            nf = 1 / (2 * np.pi) ** (D / 2) / np.prod(lam)                           # :56
            for k in range(K):
                d2 = np.sum(((X - mu_t[k]) / (sigma[k] * lam)) ** 2, axis=1)         # :59
                nn = nf * w[k] / sigma[k] ** D * np.exp(-0.5 * d2)                   # :60
                y = y + nn
                if grad:
                    dy = dy - nn[:, None] * ((X - mu_t[k]) / (lam ** 2 * sigma[k] ** 2))   # :63-64
        elif df > 0:
            nf = np.exp(gammaln((df + D) / 2) - gammaln(df / 2)) / (df * np.pi) ** (D / 2) / np.prod(lam)   # :75
            for k in range(K):
                d2 = np.sum(((X - mu_t[k]) / (sigma[k] * lam)) ** 2, axis=1)
                y = y + nf * w[k] / sigma[k] ** D * (1 + d2 / df) ** (-(df + D) / 2)   # :79
        else:
            df = abs(df)
            nf = (np.exp(gammaln((df + 1) / 2) - gammaln(df / 2)) / np.sqrt(df * np.pi)) ** D / np.prod(lam)   # :93
            for k in range(K):
                d2 = ((X - mu_t[k]) / (sigma[k] * lam)) ** 2
                y = y + nf * w[k] / sigma[k] ** D * np.prod((1 + d2 / df) ** (-(df + 1) / 2), axis=1)   # :97
        if logflag:
            if grad:
                dy = dy / y[:, None]                                                 # :108
            y = np.log(y)
        if origflag and tr:
            y = y - warp(X, "l", tr) if logflag else y / warp(X, "p", tr)            # :113-123
    return (y, dy) if grad else y


# ---------------------------------------------------------------------------------------------------------------- vbmc_rnd
def _philox(c, k0, k1):
    c = [int(v) for v in c]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def perm(seed, M, N):
    """The keyed bijection pi of [0, M) standing for randperm(numel(I), N) (:77): a six-round Feistel network on 2 hb bits, the round
    function an integer mix keyed by Philox words of the seed, with cycle walking; row r is sample pi(r)."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    c0, c1 = _philox([0, 0, 0, 4], k0, k1), _philox([1, 0, 0, 4], k0, k1)
    keys = c0 + c1[:2]
    hb = 1
    while (1 << (2 * hb)) < M:
        hb += 1
    mask = np.uint64((1 << hb) - 1)
    m32 = np.uint64(0xFFFFFFFF)

    def mix(r, k):
        p = np.uint64(0xD2511F53) * (r ^ np.uint64(k))
        h = ((p >> np.uint64(32)) ^ p) & m32
        h = ((h ^ np.uint64(k)) * np.uint64(0xCD9E8D57)) & m32
        return h ^ (h >> np.uint64(15))

    x = np.arange(N, dtype=np.uint64)
    todo = np.ones(N, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint64(hb), v & mask
        for k in keys:
            L, R = R, L ^ (mix(R, k) & mask)
        v = (L << np.uint64(hb)) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(M)
    return x.astype(np.int64)


def catrnd(cdf, u):
    """:118-123: sum(cdf < u cdf(end)) (+ 1 in the reference: components count from 0 here)"""
    return np.sum(cdf[None, :] < (u * cdf[-1])[:, None], axis=1)


def split(w, N, balanceflag, u):
    """Component of every sample id (:57-80).  u: slot 0 of every sample.  Returns (I_all, M0): I_all has M entries."""
    w = np.ravel(np.asarray(w, dtype=np.float64))
    K = w.size
    if not balanceflag:
        return np.minimum(catrnd(np.cumsum(w), u[:N]), K - 1), 0
    n_floor = np.floor(w * N)                                                        # :59
    I = np.repeat(np.arange(K), n_floor.astype(int))                                 # :60-64
    M0 = I.size
    if N > M0:
        w_extra = w * N - n_floor                                                    # :68
        s = np.cumsum(w_extra)[-1]
        n_extra = int(np.ceil(s))                                                    # :69
        w_extra = w_extra + w * (n_extra - s)                                        # :70-71
        I = np.concatenate([I, np.minimum(catrnd(np.cumsum(w_extra), u[M0:M0 + n_extra]), K - 1)])   # :72-73
    return I, M0


def catrnd_margin(w, N, balanceflag, u):
    """Smallest relative distance of a catrnd decision from a cumulative weight"""
    w = np.ravel(np.asarray(w, dtype=np.float64))
    if not balanceflag:
        cdf, uu = np.cumsum(w), u[:N]
    else:
        n_floor = np.floor(w * N)
        M0 = int(n_floor.sum())
        if N <= M0:
            return np.inf
        w_extra = w * N - n_floor
        s = np.cumsum(w_extra)[-1]
        n_extra = int(np.ceil(s))
        cdf, uu = np.cumsum(w_extra + w * (n_extra - s)), u[M0:M0 + n_extra]
    return float(np.min(np.abs(cdf[None, :] - (uu * cdf[-1])[:, None])) / cdf[-1])


def rnd(vp, N, origflag, balanceflag, B, seed):
    """[X, I] of vbmc_rnd(vp, N, origflag, balanceflag) on the block B (M x (D + 1)); also the transformed-space rows"""
    D, K = int(vp["D"]), int(vp["K"])
    I_all, _ = split(vp["w"], N, balanceflag, B[:, 0])
    pi = perm(seed, I_all.size, N) if balanceflag else np.arange(N)
    I = I_all[pi]
    Z = B[pi, 1:]
    mu_t = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K).T
    sigma, lam = np.ravel(vp["sigma"]), np.ravel(vp["lambda"])
    Y = mu_t[I] + lam[None, :] * (Z * sigma[I][:, None])                             # :84
    X = warp(Y, "i", vp.get("trinfo")) if origflag else Y                            # :102-105
    return X, I, Y


# ---------------------------------------------------------------------------------------------------------------- moments, kldiv
def moments(X):
    return np.mean(X, axis=0), np.atleast_2d(np.cov(X, rowvar=False))                # vbmc_moments.m:25-27


def kldiv_terms(vp1, vp2, xx1, xx2):
    """:70-88 given the draws; also the share of draws of each direction on which the floor rule of :76 / :82 acted"""
    MINP = np.finfo(np.float64).tiny
    out, share = [], []
    for own, oth, xx in ((vp1, vp2, xx1), (vp2, vp1, xx2)):
        qo, qt = pdf(own, xx, True), pdf(oth, xx, True)                              # :73-74 / :80-81
        qo = np.where((qo == 0) | ~np.isfinite(qo), 1.0, qo)                         # :75 / :83
        floor = (qt == 0) | ~np.isfinite(qt)
        qt = np.where(floor, MINP, qt)                                               # :76 / :82
        out.append(-np.mean(np.log(qt) - np.log(qo)))                                # :77 / :84
        share.append(float(np.mean(floor)))
    return np.maximum(np.array(out), 0.0), share                                     # :88


def mvnkl(mu1, S1, mu2, S2):
    mu1, mu2 = np.ravel(mu1), np.ravel(mu2)
    D = mu1.size
    dmu = mu2 - mu1
    lndet = np.log(np.linalg.det(S2) / np.linalg.det(S1))                            # mvnkl.m:10-12
    kl1 = 0.5 * (np.trace(np.linalg.solve(S2, S1)) + dmu @ np.linalg.solve(S2, dmu) - D + lndet)   # :14
    kl2 = 0.5 * (np.trace(np.linalg.solve(S1, S2)) + dmu @ np.linalg.solve(S1, dmu) - D - lndet)   # :16
    return kl1, kl2


def moments_analytic(vp):
    """vbmc_moments.m:30-43"""
    D, K = int(vp["D"]), int(vp["K"])
    w, mu = np.ravel(vp["w"]), np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)
    mubar = mu @ w
    S = np.sum(w * np.ravel(vp["sigma"]) ** 2) * np.diag(np.ravel(vp["lambda"]) ** 2)
    for k in range(K):
        dk = (mu[:, k] - mubar)[:, None]
        S = S + w[k] * (dk @ dk.T)
    return mubar, S


# ---------------------------------------------------------------------------------------------------------------- the test cases
CASES = {   # name: (D, K, transform types or None, scale + rotation)
    "A": (1, 1, None, False),
    "B": (4, 3, [0, 1, 2, 3], False),
    "C": (3, 4, [3, 0, 3], True),
    "D": (10, 50, [0, 3] * 5, False),
    "E": (32, 72, [3] * 16 + [0] * 16, False),
    "F": (2, 512, [0, 3], False),
    # every padded width DT and, for DT >= 8, a component count past the chunk of 2048 / DT (tests/test_vptools_restatement.py asserts both)
    "G": (5, 3, [3, 0, 1, 2, 3], True),                       # DT = 8 partly filled, a rotation with padding
    "H": (8, 257, [0, 3] * 4, False),                         # DT = 8 full, chunks 256 + 1
    "I": (12, 171, [3] * 6 + [0] * 6, True),                  # DT = 12 full with a rotation, chunks 170 + 1
    "J": (13, 4, [d % 4 for d in range(13)], True),           # DT = 16 partly filled
    "K": (16, 129, [0, 3] * 8, True),                         # DT = 16 full with a rotation, chunks 128 + 1
    "L": (17, 5, [(d + 1) % 4 for d in range(17)], True),     # DT = 24 partly filled
    "M": (24, 171, [0, 3] * 12, False),                       # DT = 24 full, chunks 85 + 85 + 1
    "N": (25, 2, [(d + 2) % 4 for d in range(25)], True),     # DT = 32 partly filled: a 25 x 25 rotation in a 32 x 32 block
    "O": (32, 512, [3] * 16 + [0] * 16, True),                # both limits: eight chunks of 64, the rotation at the largest LDS footprint
}
PADDED_WIDTHS = (4, 8, 12, 16, 24, 32)   # vpt_pick_dt (vbmc_amd/csrc/vp_tools_host.h): the smallest of these that holds D
CHUNK_DOUBLES = 2048                     # VPT_CHUNK (vbmc_amd/csrc/vp_tools_kernels.h): 2048 / DT components are staged at a time


def padded_width(D):
    return next(dt for dt in PADDED_WIDTHS if D <= dt)
POINT_COUNTS = (1, 63, 64, 65, 1003)


def make_vp(D, K, types, rot, seed=1, width=1.0):
    r = np.random.default_rng(seed)
    mu = r.normal(0, 1, (D, K))
    sigma = np.exp(r.normal(-1, .3, K)) * width
    lam = np.exp(r.normal(0, .3, D))
    lam /= np.sqrt(np.mean(lam ** 2))
    w = r.dirichlet(np.ones(K))
    vp = dict(D=D, K=K, mu=mu, sigma=sigma, w=w, trinfo=None)
    vp["lambda"] = lam
    if types is not None:
        lb, ub = np.full(D, -np.inf), np.full(D, np.inf)
        tmu, tdel = r.normal(0, .3, D), np.exp(r.normal(0, .3, D))
        for d, t in enumerate(types):
            if t in (1, 3):
                lb[d] = r.uniform(-2, 0)
            if t in (2, 3):
                ub[d] = r.uniform(1, 4)
            if t in (1, 2):
                tmu[d], tdel[d] = 0.0, 1.0
        tr = dict(lb_orig=lb, ub_orig=ub, type=np.array(types), mu=tmu, delta=tdel, scale=None, R_mat=None)
        if rot:
            tr["R_mat"], _ = np.linalg.qr(r.normal(size=(D, D)))
            tr["scale"] = np.exp(r.normal(0, .2, D))
        vp["trinfo"] = tr
    return vp


# ---- small posteriors for the transform's edges (tests/test_gpu_vptools_edges.py): no rotation, so that a row differs from an
# ordinary one in exactly one transformed coordinate; a wide component (sigma = 8) sits where the edge rows land, so that the density
# there is finite and depends on the transformed coordinate
def make_zero_bounds():
    """D = 3, K = 3: a type-1 variable with lb_orig = 0, a type-2 variable with ub_orig = 0 (only next to a bound at 0 does
    x - a become subnormal), a type-0 variable; wide components at log(x - a) = -725 and at log(b - x) = -725"""
    inf = np.inf
    tr = dict(lb_orig=np.array([0.0, -inf, -inf]), ub_orig=np.array([inf, 0.0, inf]), type=np.array([1, 2, 0]), mu=np.array([0.0, 0.0, 0.3]),
              delta=np.array([1.0, 1.0, 1.2]), scale=None, R_mat=None)
    vp = dict(D=3, K=3, mu=np.array([[-0.5, -725.0, 0.0], [0.2, 0.0, -725.0], [0.1, 0.0, 0.0]]), sigma=np.array([0.5, 8.0, 8.0]),
              w=np.array([0.5, 0.25, 0.25]), trinfo=tr)
    vp["lambda"] = np.array([1.0, 1.1, 0.9])
    return vp


def make_logit():
    """D = 2, K = 3: a logit variable on (-1, 3) and a type-0 variable; wide components at logit z = 0.2, 725 and 1e4"""
    tr = dict(lb_orig=np.array([-1.0, -np.inf]), ub_orig=np.array([3.0, np.inf]), type=np.array([3, 0]), mu=np.array([0.2, -0.1]),
              delta=np.array([1.3, 0.8]), scale=None, R_mat=None)
    vp = dict(D=2, K=3, mu=np.array([[0.0, (725.0 - 0.2) / 1.3, (1e4 - 0.2) / 1.3], [-0.2, 0.0, 0.0]]), sigma=np.array([8.0, 8.0, 8.0]),
              w=np.array([0.5, 0.3, 0.2]), trinfo=tr)
    vp["lambda"] = np.array([1.0, 1.0])
    return vp


def _rows(base, changes):
    X = np.repeat(np.asarray(base, dtype=np.float64)[None, :], len(changes) + 1, axis=0)     # row 0 stays ordinary
    for i, (d, v) in enumerate(changes):
        X[i + 1, d] = v
    return X


def zero_bounds_rows():
    """Original-space rows of make_zero_bounds(): (near, huge, on a bound, outside a bound); each differs from the ordinary first
    row in one coordinate"""
    base = [np.exp(-0.3), -np.exp(0.4), 0.5]
    near = _rows(base, [(0, 2.0 ** -1060), (0, 2.0 ** -1030), (1, -2.0 ** -1060), (1, -2.0 ** -1030)])   # x - a resp. b - x subnormal
    huge = _rows(base, [(2, 1e160), (2, -1e160), (2, 1e200), (2, -1e200)])                                # the squared distance overflows
    on = _rows(base, [(0, 0.0), (1, 0.0)])
    out = _rows(base, [(0, -0.5), (1, 0.5), (0, -2.0 ** -1060), (1, 2.0 ** -1060)])
    return near, huge, on, out


def logit_rows():
    """Original-space rows of make_logit(): (z next to 0 and to 1, huge, on a bound, outside a bound)"""
    base = [0.7, 0.4]
    near = _rows(base, [(0, -1.0 + 2.0 ** -38), (0, -1.0 + 2.0 ** -50), (0, 3.0 - 2.0 ** -38), (0, 3.0 - 2.0 ** -50)])   # z = 2^-40, 2^-52, 1 - ...
    huge = _rows(base, [(1, 1e160), (1, -1e160), (1, 1e200), (1, -1e200)])
    on = _rows(base, [(0, -1.0), (0, 3.0)])
    out = _rows(base, [(0, -1.5), (0, 3.5), (0, np.nextafter(-1.0, -2.0)), (0, np.nextafter(3.0, 4.0))])
    return near, huge, on, out


LOGIT_Z = (30.0, 37.0, 40.0, 700.0, 750.0, 1e4)   # 37: 1 + exp(-z) rounds to 1; 745: exp(-z) is 0
LOGIT_Z_REF_OVERFLOWS = 709.782712893384        # below -log(realmax) the reference's exp(-z) is Inf and its log-Jacobian -Inf


def logit_trans_rows(vp, zs):
    """Transformed-space rows of make_logit() whose logit coordinate is z = y delta + mu for the given z (the first row ordinary)"""
    tr = vp["trinfo"]
    return _rows([0.3, -0.2], [(0, (z - tr["mu"][0]) / tr["delta"][0]) for z in zs])


def make_clamp():
    """D = 4, types 0 .. 3, components wide enough that a normal of +-1e3 takes exp() past its range in both directions"""
    vp = make_vp(4, 3, [0, 1, 2, 3], False)
    vp["sigma"] = np.array([1.5, 2.0, 2.5])
    return vp


CLAMP_ROWS = ((3, 1e3), (7, -1e3), (20, 1e3), (41, -1e3))   # output rows of vbmc_rnd whose D normals are set to the value


def clamp_block(B, perm):
    """The dumped block with the normals of the samples behind CLAMP_ROWS replaced"""
    B = np.array(B)
    for r, v in CLAMP_ROWS:
        B[perm[r], 1:] = v
    return B


def make_zero_weight(which):
    """D = 5 with the transform of case G, K = 4; the weights of ``which`` are zero (and the others sum to one)"""
    D, K, types, rot = CASES["G"]
    vp = make_vp(D, 4, types, rot)
    w = np.array(vp["w"])
    w[list(which)] = 0.0
    vp["w"] = w / w.sum()
    return vp


ZERO_WEIGHTS = ((0,), (2,), (0, 1, 2))


def make_case(name, seed=1, width=1.0):
    D, K, types, rot = CASES[name]
    return make_vp(D, K, types, rot, seed, width)


def far_point(vp):
    """An original-space point (1 x D) whose transformed-space density underflows while every transform stays finite: the image of
    the mixture mean, moved by 200 in every unbounded (type 0) coordinate"""
    D, K = int(vp["D"]), int(vp["K"])
    tr = vp.get("trinfo")
    x = warp((np.asarray(vp["mu"]).reshape(D, K) @ np.ravel(vp["w"]))[None, :], "i", tr)
    free = np.ones(D, dtype=bool) if not tr else np.asarray(tr["type"]) == 0
    x[:, free] += 200.0
    return x


def sibling(vp, seed=2, width=1.0, same_mu=False):
    """Another posterior on the same bounds: other means, widths and weights, and another mu / delta of the transform"""
    D, K = int(vp["D"]), int(vp["K"])
    r = np.random.default_rng(seed)
    out = dict(vp)
    out["mu"] = np.asarray(vp["mu"]) + (0.0 if same_mu else 0.3) * r.normal(size=(D, K))
    out["sigma"] = np.ravel(vp["sigma"]) * width * np.exp(r.normal(0, .1, K))
    out["w"] = r.dirichlet(np.ones(K) * 3)
    if vp.get("trinfo"):
        tr = dict(vp["trinfo"])
        free = np.isin(np.asarray(tr["type"]), (0, 3))
        tr["mu"] = np.where(free, np.ravel(tr["mu"]) + 0.2 * r.normal(size=D), tr["mu"])
        tr["delta"] = np.where(free, np.ravel(tr["delta"]) * np.exp(0.2 * r.normal(size=D)), tr["delta"])
        out["trinfo"] = tr
    return out


NARROW = dict(case="B", width=0.08)   # vbmc_kldiv.m:76 acts on a share of vp1's draws (tests/test_vptools_restatement.py asserts 1-20 %)

"""NumPy / SciPy restatement of the numerics of utils/cornerplot.m:113-156 with utils/kde2d.m:74-212 and utils/quantile1.m:37-72, line by
line, on a given sample matrix (so that it can be fed the device's own draws).  Every stage is returned.

Where it follows vbmc_vp_corner (include/vbmc_hip.h) instead of the reference, on purpose:
  * the histogram of a dimension has nbins equal bins between its bounds, edge k at lo + k (hi - lo) / nbins (cornerplot.m:129 calls
    histogram(x, 40), whose "nice" edges are toolbox code outside the reference tree);
  * the root of t - evolve(t) comes from brentq at its tightest tolerances inside the bracket root() (kde2d.m:196-212) arrives at; no
    bracket below 0.1 (the fminbnd branch, :208-210) raises NoBracket."""
import numpy as np

from tests._mtv_ref import EPS, NoBracket, bracket, root  # noqa: F401  (root() of kde2d.m:196-212 is kde1d.m:124-140's)


# ---------------------------------------------------------------------------------------------------------------- kde2d.m
def dct2d(data):
    """kde2d.m:142-161"""
    data = np.asarray(data, dtype=np.float64)
    nrows = data.shape[0]
    w = np.concatenate(([1.0], 2.0 * np.exp(-1j * np.arange(1, nrows) * np.pi / (2 * nrows))))     # :150
    weight = w[:, None]

    def dct1d(x):
        x = np.concatenate((x[0::2, :], x[::-1, :][0::2, :]), axis=0)                            # :156: x(1:2:end,:); x(end:-2:2,:)
        return np.real(weight * np.fft.fft(x, axis=0))                                            # :159
    return dct1d(dct1d(data).T).T                                                                 # :152


def idct2d(data):
    """kde2d.m:163-176"""
    data = np.asarray(data, dtype=np.float64)
    nrows = data.shape[0]
    weights = np.exp(1j * np.arange(nrows) * np.pi / (2 * nrows))[:, None]                        # :167

    def idct1d(x):
        y = np.real(np.fft.ifft(weights * x, axis=0))                                             # :171
        out = np.zeros_like(y)
        out[0::2, :] = y[: nrows // 2, :]                                                         # :173
        out[1::2, :] = y[::-1, :][: nrows // 2, :]                                                # :174: y(nrows:-1:nrows/2+1,:)
        return out
    return idct1d(idct1d(data).T)                                                                 # :169: one transpose


def _cosmat(n):
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return np.cos(np.pi * k * (2 * j + 1) / (2 * n))                                              # c(k, j)


def dct2d_sum(x):
    """a = C x C', C(k, j) = f_k cos(pi k (2 j + 1) / (2 n)), f_0 = 1, f_k = 2: what dct2d stands for"""
    n = x.shape[0]
    C = _cosmat(n) * np.where(np.arange(n) == 0, 1.0, 2.0)[:, None]
    return C @ x @ C.T


def idct2d_sum(a):
    """out(j2, j1) = sum_{k1, k2} a(k1, k2) c(k1, j1) c(k2, j2) / n^2: what idct2d stands for (transposed)"""
    n = a.shape[0]
    C = _cosmat(n)
    return (C.T @ a @ C).T / n ** 2


def ndhist_bins(t, M):
    """histc(t, 0:1/M:1) followed by min(., M) (kde2d.m:188-189): 1 .. M, 0 for what lies outside [0, 1] or is not a number"""
    edges = np.arange(M + 1) / M
    b = np.searchsorted(edges, t, side="right")
    b = np.where(np.isnan(t) | (t < 0) | (t > 1), 0, b)
    return np.minimum(b, M)


def ndhist(data, M):
    """kde2d.m:178-194: (binned_data, counts)"""
    nrows = data.shape[0]
    bins = np.stack([ndhist_bins(data[:, i], M) for i in range(2)], axis=1)
    keep = np.all(bins > 0, axis=1)                                                               # :193
    counts = np.zeros((M, M), dtype=np.int64)
    np.add.at(counts, (bins[keep, 0] - 1, bins[keep, 1] - 1), 1)
    return counts * (1 / nrows), counts


def K(s):
    return (-1) ** s * np.prod(np.arange(1, 2 * s, 2, dtype=np.float64)) / np.sqrt(2 * np.pi)    # :139


def psi(s, Time, I, A2):
    """kde2d.m:129-136"""
    with np.errstate(all="ignore"):
        w = np.exp(-I * np.pi ** 2 * Time) * np.concatenate(([1.0], .5 * np.ones(I.size - 1)))   # :132
        wx = w * I ** s[0]                                                                        # :133
        wy = w * I ** s[1]                                                                        # :134
        return (-1) ** sum(s) * (wy @ A2 @ wx) * np.pi ** (2 * sum(s))                            # :135


def _time(s, N, Sum_func):
    with np.errstate(all="ignore"):
        const = (1 + 1 / 2 ** (sum(s) + 1)) / 3                                                   # :120
        base = np.float64(-2 * const * K(s[0]) * K(s[1]) / N) / np.float64(Sum_func)
        return np.float64(base) ** (1 / (2 + sum(s))) if base >= 0 else np.nan                    # :121


def func(s, t, N, I, A2, count=None):
    """kde2d.m:117-127, the plain recursion"""
    if count is not None:
        count[0] += 1
    if sum(s) <= 4:
        Sum_func = func((s[0] + 1, s[1]), t, N, I, A2, count) + func((s[0], s[1] + 1), t, N, I, A2, count)
        return psi(s, _time(s, N, Sum_func), I, A2)
    return psi(s, t, I, A2)


def func_dag(t, N, I, A2):
    """func at the 18 distinct nodes, level by level from the leaves [i, 5 - i]: {s: value}.  A node's value depends on (s, t) only
    and every addition keeps func's order, so this is what the recursion returns."""
    val = {(i, 5 - i): psi((i, 5 - i), t, I, A2) for i in range(6)}
    for L in range(4, 1, -1):
        for i in range(L + 1):
            s = (i, L - i)
            val[s] = psi(s, _time(s, N, val[(i + 1, L - i)] + val[(i, L - i + 1)]), I, A2)
    return val


def evolve(t, N, I, A2, f=None):
    """kde2d.m:110-115: (out, time)"""
    v = func_dag(t, N, I, A2) if f is None else {s: f(s, t, N, I, A2) for s in ((0, 2), (2, 0), (1, 1))}
    with np.errstate(all="ignore"):
        Sum_func = v[(0, 2)] + v[(2, 0)] + 2 * v[(1, 1)]                                          # :112
        base = np.float64(2 * np.pi * N * Sum_func)
        time = base ** (-1 / 3) if base >= 0 else np.nan                                          # :113
        return (t - time) / time, time                                                            # :114


def kde2d(data, n, MIN_XY, MAX_XY):
    """kde2d.m:74-108 with given bounds: a dict with bandwidth, density, tstar and the stages"""
    data = np.asarray(data, dtype=np.float64)
    N = data.shape[0]                                                                             # :79
    MIN_XY, MAX_XY = np.asarray(MIN_XY, dtype=np.float64), np.asarray(MAX_XY, dtype=np.float64)
    scaling = MAX_XY - MIN_XY                                                                     # :84
    with np.errstate(all="ignore"):
        transformed = (data - MIN_XY[None, :]) / scaling[None, :]                                 # :88
    initial_data, counts = ndhist(transformed, n)                                                 # :90
    a = dct2d(initial_data)                                                                       # :92
    I = np.arange(n, dtype=np.float64) ** 2                                                       # :94
    A2 = a ** 2
    f = lambda t: t - evolve(t, N, I, A2)[0]                                                      # :95
    t_star, tol = root(f, N)
    v = func_dag(t_star, N, I, A2)
    p_02, p_20, p_11 = v[(0, 2)], v[(2, 0)], v[(1, 1)]                                            # :96
    t_y = (p_02 ** (3 / 4) / (4 * np.pi * N * p_20 ** (3 / 4) * (p_11 + np.sqrt(p_20 * p_02)))) ** (1 / 3)   # :97
    t_x = (p_20 ** (3 / 4) / (4 * np.pi * N * p_02 ** (3 / 4) * (p_11 + np.sqrt(p_20 * p_02)))) ** (1 / 3)   # :98
    k = np.arange(n, dtype=np.float64)
    a_t = np.outer(np.exp(-k ** 2 * np.pi ** 2 * t_x / 2), np.exp(-k ** 2 * np.pi ** 2 * t_y / 2)) * a       # :100
    density = idct2d(a_t) * (a_t.size / np.prod(scaling))                                         # :103
    density[density < 0] = EPS                                                                    # :104
    bandwidth = np.sqrt(np.array([t_x, t_y])) * scaling                                           # :107
    return dict(bandwidth=bandwidth, density=density, tstar=t_star, counts2=counts, a=a, A2=A2, I=I, N=N, tol=tol, t_x=t_x, t_y=t_y, f=f)


# ---------------------------------------------------------------------------------------------------------------- quantile1.m
def quantile_ranks(p, n):
    """(k, kp1, r) of quantile1.m:47-54, ranks from 1"""
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    r = p * n                                                                                      # :47
    k = np.floor(r + 0.5)                                                                          # :48
    kp1 = k + 1                                                                                    # :49
    r = r - k                                                                                      # :50
    k = np.where(k < 1, 1, k)                                                                      # :53
    kp1 = np.minimum(kp1, n)                                                                       # :54
    return k.astype(np.int64), kp1.astype(np.int64), r


def quantile1(x, p):
    """quantile1.m:37-72 on one column without NaN"""
    x = np.sort(np.ravel(np.asarray(x, dtype=np.float64)))                                         # :37
    n = x.size
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if p.size == 1 and p[0] == 0.5:                                                                # :40
        if n % 2:
            return np.array([x[(n + 1) // 2 - 1]])                                                 # :42
        return np.array([(x[n // 2 - 1] + x[n // 2]) / 2])                                         # :44
    k, kp1, r = quantile_ranks(p, n)
    y = (0.5 + r) * x[kp1 - 1] + (0.5 - r) * x[k - 1]                                              # :57
    exact = r == -0.5                                                                              # :60
    y[exact] = x[k[exact] - 1]
    same = x[k - 1] == x[kp1 - 1]                                                                  # :66
    y[same] = x[k[same] - 1]
    return y


# ---------------------------------------------------------------------------------------------------------------- cornerplot.m
def hist1(x, lo, hi, nbins):
    """Counts on nbins equal bins of [lo, hi]: bin k the largest k with lo + k (hi - lo) / nbins <= x, a sample on hi in the last
    bin, samples outside not counted"""
    w = (hi - lo) / nbins
    edges = lo + np.arange(nbins) * w
    x = x[(x >= lo) & (x <= hi)]
    k = np.clip(np.searchsorted(edges, x, side="right") - 1, 0, nbins - 1)
    return np.bincount(k, minlength=nbins).astype(np.int64)


def pair_list(D):
    return [(d1, d2) for d1 in range(D - 1) for d2 in range(d1 + 1, D)]                            # cornerplot.m:154-155


def corner(X, bounds=None, res=64, nbins=40, p=(0.5,)):
    """cornerplot.m:113-156's numbers for the sample matrix X (Ns x D).  bounds: None (the columns' min and max, :93-96, :116) or
    (D, 2).  Returns a dict: bounds (D, 2), hist (D, nbins), quant (D, nq), pairs, and per pair density (P, res, res; row the d2
    mesh, column the d1 mesh), bandwidth (P, 2), tstar (P), counts2 (P, res, res; row the d1 bin), tol (P), kde (the stage dicts).  A
    column of zero range without given bounds has a zero histogram and NaN in its pairs."""
    X = np.asarray(X, dtype=np.float64)
    Ns, D = X.shape
    b = np.stack([np.min(X, axis=0), np.max(X, axis=0)], axis=1) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(D, 2)
    bad = ~((b[:, 1] - b[:, 0] > 0) & np.isfinite(b[:, 1] - b[:, 0]))
    out = dict(bounds=b, pairs=pair_list(D))
    out["hist"] = np.stack([np.zeros(nbins, dtype=np.int64) if bad[d] else hist1(X[:, d], b[d, 0], b[d, 1], nbins) for d in range(D)])
    out["quant"] = np.stack([quantile1(X[:, d], p) for d in range(D)]) if len(p) else np.zeros((D, 0))
    P = len(out["pairs"])
    out.update(density=np.full((P, res, res), np.nan), bandwidth=np.full((P, 2), np.nan), tstar=np.full(P, np.nan),
               counts2=np.zeros((P, res, res), dtype=np.int64), tol=np.zeros(P), kde=[None] * P)
    for pp, (d1, d2) in enumerate(out["pairs"]):
        if bad[d1] or bad[d2]:
            with np.errstate(all="ignore"):
                t = (X[:, [d1, d2]] - b[[d1, d2], 0][None, :]) / (b[[d1, d2], 1] - b[[d1, d2], 0])[None, :]
            out["counts2"][pp] = ndhist(t, res)[1]
            continue
        k = kde2d(X[:, [d1, d2]], res, b[[d1, d2], 0], b[[d1, d2], 1])                             # :156
        out["density"][pp], out["bandwidth"][pp], out["tstar"][pp], out["counts2"][pp], out["tol"][pp] = k["density"], k["bandwidth"], k["tstar"], k["counts2"], k["tol"]
        out["kde"][pp] = k
    return out


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases
SEED = 20241021


def _gauss(D, K, seed):
    r = np.random.default_rng(seed)
    vp = dict(D=D, K=K, mu=r.normal(0, 1, (D, K)), sigma=np.exp(r.normal(-0.5, .2, K)), w=r.dirichlet(np.ones(K) * 4), trinfo=None)
    vp["lambda"] = np.exp(r.normal(0, .3, D))
    return vp


def make_pile():
    """tests/_mtv_ref.make_pile with a milder first dimension: some hundred of 4097 draws sit on each clamp end of the logit variable
    (ties for the selection), the rest spread over (-1, 3)"""
    from tests import _mtv_ref

    vp = _mtv_ref.make_pile()
    vp["sigma"] = np.array([30.0, 25.0, 20.0])
    vp["mu"] = np.array([[0.0, 2.0, -2.0], [-0.2, 0.0, 0.3]])
    return vp


def make_case(name):
    """(vp, Ns, res, bounds, balanceflag) of a posterior case.  bounds: None or (D, 2)."""
    from tests import _vptools_ref as T

    if name == "small":        # one pair, fewer samples than a workgroup
        return _gauss(2, 1, 3), 67, 16, None, 0
    if name in ("three32", "three64"):   # odd Ns, three pairs with unequal marginals: pair order and transposition
        vp = _gauss(3, 4, 4)
        vp["lambda"] = np.array([0.4, 1.0, 2.5])
        return vp, 1003, 32 if name == "three32" else 64, None, 0
    if name in ("cut0", "cut1"):         # given bounds that cut the samples; logit bounds, scale and rotation; balance 0 and 1
        vp = T.make_case("G")
        return vp, 5000, 64, "cut", 0 if name == "cut0" else 1
    if name == "wide32":       # 496 pairs, D x res indexing
        return _gauss(32, 3, 5), 2000, 16, None, 0
    if name == "pile":         # draws piled on the clamp ends
        return make_pile(), 4097, 32, None, 1
    if name == "one":          # D = 1: no pairs
        return _gauss(1, 2, 6), 1003, 64, None, 0
    raise KeyError(name)


def cut_bounds(X, lo=0.2, hi=0.85):
    """Bounds at the given quantiles of every column of X: they keep hi - lo of each marginal"""
    return np.stack([np.quantile(X, lo, axis=0), np.quantile(X, hi, axis=0)], axis=1)


VP_CASES = ("small", "three32", "three64", "cut0", "cut1", "wide32", "pile", "one")
QUANT_P = (0.5, 0.025, 0.25, 0.975, 0.0, 1.0, 1e-5)


def edge_matrix():
    """(X, bounds): a given matrix of 1003 x 2 correlated Gaussian samples with rows exactly on both bounds of either dimension and
    rows outside them"""
    r = np.random.default_rng(SEED)
    X = r.normal(0, 1, (1003, 2)) @ np.array([[1.0, 0.6], [0.0, 0.8]])
    b = np.array([[-2.5, 2.5], [-2.0, 2.25]])
    X[0] = [-2.5, 0.1]; X[1] = [2.5, -0.3]; X[2] = [0.2, -2.0]; X[3] = [-0.4, 2.25]; X[4] = [2.5, 2.25]; X[5] = [-2.5, -2.0]
    X[6] = [-2.6, 0.0]; X[7] = [0.0, 2.3]; X[8] = [3.0, -3.0]
    return X, b


def small_cut():
    """(X, bounds): 300 x 2 Gaussian samples cut by bounds to about a third of their mass -- no bracket below 0.1 (the refusal)"""
    r = np.random.default_rng(SEED + 1)
    X = r.normal(0, 1, (300, 2))
    return X, np.array([[-0.3, 0.6], [-0.5, 0.4]])


def case_draws(name):
    """(X, res, bounds) of a posterior case on the restatement's own draws: tests/_vptools_ref.rnd on the block the seed stands for (a
    host function: no device), which the device's draws equal to a few ulps"""
    from tests import _vptools_ref as T
    from vbmc_amd import vptools

    vp, Ns, res, bounds, bal = make_case(name)
    B, _ = vptools.vp_rnd_rng_dump(SEED, Ns, vp["D"], vp["w"], bool(bal))
    X = T.rnd(vp, Ns, True, bool(bal), B, SEED)[0]
    return X, res, (cut_bounds(X) if isinstance(bounds, str) else bounds)

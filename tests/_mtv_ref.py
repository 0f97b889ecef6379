"""NumPy / SciPy restatement of vbmc_mtv.m:24-79 with shared/kde1d.m:35-140 and shared/qtrapz.m, line by line, on given sample
matrices (so that it can be fed the device's own draws: moving one sample of 1e5 across a bin edge moves the result by 1e-7, and
identical inputs are the only way to a tight comparison).  Every stage is returned.

Where it follows vbmc_vp_mtv (include/vbmc_hip.h) instead of the reference, on purpose:
  * the mesh is e_k = MIN + k dx, k = 0 .. n - 1 (kde1d.m:46 writes MIN + [0:dx:R], whose last point is a matter of the colon
    operator's rounding), and a sample at or beyond e_{n-1} goes to the last bin;
  * N = length(unique(data)) (:46) is taken as given by ``nuniq`` (the device's clamp-end rule) or, by default, by np.unique;
  * the root of fixed_point comes from brentq at its tightest tolerances inside the bracket root() (:124-140) arrives at; no bracket
    below 0.1 (the fminbnd branch, :136-138) raises NoBracket."""
import numpy as np
from scipy.interpolate import CubicSpline
from scipy.optimize import brentq

EPS = np.finfo(np.float64).eps


class NoBracket(Exception):
    """root() reached tol == 0.1 (kde1d.m:136-138)"""


def qtrapz(y):
    y = np.asarray(y, dtype=np.float64)
    return np.sum(y) - 0.5 * (y[0] + y[-1])                                           # qtrapz.m:34


def dct1d(data):
    """kde1d.m:113-122"""
    data = np.asarray(data, dtype=np.float64)
    nrows = data.size
    weight = np.concatenate(([1.0], 2.0 * np.exp(-1j * np.arange(1, nrows) * np.pi / (2 * nrows))))   # :117
    data = np.concatenate((data[0::2], data[::-1][0::2]))                                               # :119: data(1:2:end); data(end:-2:2)
    return np.real(weight * np.fft.fft(data))                                                           # :121


def idct1d(data):
    """kde1d.m:94-110"""
    data = np.asarray(data, dtype=np.float64)
    nrows = data.size
    weights = nrows * np.exp(1j * np.arange(nrows) * np.pi / (2 * nrows))             # :99
    data = np.real(np.fft.ifft(weights * data))                                        # :101
    out = np.zeros(nrows)
    out[0::2] = data[: nrows // 2]                                                     # :105
    out[1::2] = data[::-1][: nrows // 2]                                               # :106: data(nrows:-1:nrows/2+1)
    return out


def dct_sum(x):
    """a_0 = sum x_j, a_k = 2 sum_j x_j cos(pi k (2 j + 1) / (2 n)): what dct1d stands for"""
    n = x.size
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    a = 2.0 * np.cos(np.pi * k * (2 * j + 1) / (2 * n)) @ x
    a[0] = np.sum(x)
    return a


def idct_sum(a):
    """out_j = sum_k a_k cos(pi k (2 j + 1) / (2 n)): what idct1d stands for"""
    n = a.size
    j, k = np.arange(n)[:, None], np.arange(n)[None, :]
    return np.cos(np.pi * k * (2 * j + 1) / (2 * n)) @ a


def fixed_point(t, N, I, a2):
    """kde1d.m:79-89"""
    with np.errstate(all="ignore"):
        l = 7
        f = 2 * np.pi ** (2 * l) * np.sum(I ** l * a2 * np.exp(-I * np.pi ** 2 * t))  # :82
        for s in range(l - 1, 1, -1):                                                  # :83
            K0 = np.prod(np.arange(1, 2 * s, 2, dtype=np.float64)) / np.sqrt(2 * np.pi)
            const = (1 + (1 / 2) ** (s + 1 / 2)) / 3                                   # :84
            time = (2 * const * K0 / N / f) ** (2 / (3 + 2 * s))                       # :85
            f = 2 * np.pi ** (2 * s) * np.sum(I ** s * a2 * np.exp(-I * np.pi ** 2 * time))   # :86
        return t - (2 * N * np.sqrt(np.pi) * f) ** (-2 / 5)                            # :88


def bracket(f, N):
    """The interval [0, tol] on which root() (kde1d.m:124-140) calls fzero successfully: the endpoint values finite and of opposite
    signs (what fzero asks of an interval).  NoBracket where tol reaches 0.1."""
    N = 50 * (N <= 50) + 1050 * (N >= 1050) + N * ((N < 1050) & (N > 50))              # :126
    tol = 10 ** -12 + 0.01 * (N - 50) / 1000                                           # :127
    f0 = f(0.0)
    while True:
        ft = f(tol)
        if np.isfinite(f0) and np.isfinite(ft) and ((f0 <= 0 <= ft) or (ft <= 0 <= f0)):
            return tol, f0, ft
        tol = min(tol * 2, .1)                                                         # :134
        if tol == .1:                                                                  # :136
            raise NoBracket()


def root(f, N):
    tol, f0, ft = bracket(f, N)
    if f0 == 0:
        return 0.0, tol
    if ft == 0:
        return tol, tol
    return brentq(f, 0.0, tol, xtol=1e-300, rtol=4 * EPS, maxiter=1000), tol


def mesh_edges(MIN, MAX, n):
    R = MAX - MIN
    dx = R / (n - 1)                                                                   # kde1d.m:46
    return MIN + np.arange(n) * dx, R, dx


def histc(data, edges):
    k = np.searchsorted(edges, data, side="right") - 1                                 # the largest k with e_k <= x
    k = np.clip(k, 0, edges.size - 1)
    return np.bincount(k, minlength=edges.size).astype(np.int64)


def kde1d(data, n, MIN, MAX, nuniq=None):
    """kde1d.m:35-62: (t_star, density, xmesh) and the stages"""
    data = np.ravel(data)
    xmesh, R, dx = mesh_edges(MIN, MAX, n)
    N = int(np.unique(data).size if nuniq is None else nuniq)                          # :46
    counts = histc(data, xmesh)
    initial_data = counts / N                                                          # :48
    initial_data = initial_data / np.sum(initial_data)
    a = dct1d(initial_data)                                                            # :49
    I = np.arange(1, n, dtype=np.float64) ** 2                                         # :51
    a2 = (a[1:] / 2) ** 2
    f = lambda t: fixed_point(t, N, I, a2)
    t_star, tol = root(f, N)                                                           # :53
    a_t = a * np.exp(-np.arange(n, dtype=np.float64) ** 2 * np.pi ** 2 * t_star / 2)   # :55
    density = idct1d(a_t) / R                                                          # :58
    density[density < 0] = EPS                                                         # :62
    return t_star, density, xmesh, dict(counts=counts, N=N, a=a, a2=a2, I=I, tol=tol)


def mesh_bounds(xx, lb, ub):
    lo, hi = np.min(xx, axis=0), np.max(xx, axis=0)                                    # vbmc_mtv.m:55 / :60
    rng = hi - lo
    return np.maximum(lo - rng / 10, lb), np.minimum(hi + rng / 10, ub)               # :57-58 / :62-63


def spline0(xmesh, yy, x):
    """interp1(xmesh, yy, x, 'spline', 0)"""
    v = CubicSpline(xmesh, yy, bc_type="not-a-knot", extrapolate=False)(x)
    return np.where(np.isnan(v), 0.0, v)


def bounds_of(vp, D):
    tr = vp.get("trinfo") if isinstance(vp, dict) else None
    if not tr:
        return np.full(D, -np.inf), np.full(D, np.inf)
    return np.asarray(tr["lb_orig"], dtype=np.float64).ravel(), np.asarray(tr["ub_orig"], dtype=np.float64).ravel()


def clamp_rule(x, lb, ub):
    """The device's unique count: Ns - max(0, c_lo - 1) - max(0, c_hi - 1) with the clamp ends of warpvars_vbmc.m:456-459"""
    n = x.size
    if np.isfinite(lb):
        n -= max(0, int(np.sum(x == lb + np.spacing(abs(lb)))) - 1)
    if np.isfinite(ub):
        n -= max(0, int(np.sum(x == ub - np.spacing(abs(ub)))) - 1)
    return n


def mtv(xx1, xx2, lb1, ub1, lb2, ub2, nkde=2 ** 13, nquad=100000, nuniq=None):
    """vbmc_mtv.m:50-79 given the draws and the posteriors' lb_orig / ub_orig.  Returns (mtv, stages); a column whose range is zero
    or not finite gives NaN there."""
    xx1, xx2 = np.asarray(xx1, dtype=np.float64), np.asarray(xx2, dtype=np.float64)
    D = xx1.shape[1]
    out = np.zeros(D)
    lo1, hi1 = mesh_bounds(xx1, lb1, ub1)
    lo2, hi2 = mesh_bounds(xx2, lb2, ub2)
    st = dict(mesh=np.zeros((2, D, 2)), counts=np.zeros((2, D, nkde), dtype=np.int64), nuniq=np.zeros((2, D), dtype=np.int64),
              tstar=np.full((2, D), np.nan), density=np.full((2, D, nkde), np.nan), tol=np.zeros((2, D)), kde=[[None] * D, [None] * D])
    st["mesh"][0, :, 0], st["mesh"][0, :, 1], st["mesh"][1, :, 0], st["mesh"][1, :, 1] = lo1, hi1, lo2, hi2
    for i in range(D):                                                                 # :66
        mesh, yy = [], []
        for p, (xx, lo, hi) in enumerate(((xx1, lo1, hi1), (xx2, lo2, hi2))):
            rng = np.max(xx[:, i]) - np.min(xx[:, i])
            if not (rng > 0 and np.isfinite(rng) and hi[i] - lo[i] > 0 and np.isfinite(hi[i] - lo[i])):
                st["nuniq"][p, i] = np.unique(xx[:, i]).size if nuniq is None else nuniq[p, i]
                continue
            t, y, xm, k = kde1d(xx[:, i], nkde, lo[i], hi[i], None if nuniq is None else nuniq[p, i])   # :67 / :70
            y = y / (qtrapz(y) * (xm[1] - xm[0]))                                      # :68 / :71
            st["counts"][p, i], st["nuniq"][p, i], st["tstar"][p, i], st["density"][p, i], st["tol"][p, i] = k["counts"], k["N"], t, y, k["tol"]
            st["kde"][p][i] = k
            mesh.append(xm)
            yy.append(y)
        if len(mesh) < 2:
            out[i] = np.nan
            continue
        f = lambda x: np.abs(spline0(mesh[0], yy[0], x) - spline0(mesh[1], yy[1], x))  # :73
        bb = np.sort([mesh[0][0], mesh[0][-1], mesh[1][0], mesh[1][-1]])               # :74
        for j in range(3):                                                             # :75
            if not bb[j + 1] > bb[j]:
                continue
            xr = np.linspace(bb[j], bb[j + 1], nquad)                                  # :76
            out[i] += 0.5 * qtrapz(f(xr)) * (xr[1] - xr[0])                            # :77
    return out, st


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases
SEED = 20241019


def _gauss(D, mean, sd):
    vp = dict(D=D, K=1, mu=np.full((D, 1), float(mean)), sigma=np.array([float(sd)]), w=np.array([1.0]), trinfo=None)
    vp["lambda"] = np.ones(D)
    return vp


def _other_bounds(vp):
    """The same posterior on other bounds (every finite bound moved outwards)"""
    out = dict(vp)
    tr = dict(vp["trinfo"])
    tr["lb_orig"] = np.asarray(tr["lb_orig"]) - 0.7
    tr["ub_orig"] = np.asarray(tr["ub_orig"]) + 1.3
    out["trinfo"] = tr
    return out


def make_pile():
    """D = 2: a logit variable on (-1, 3) whose transformed coordinate has a standard deviation of ~2000, so that all but ~45 of 4097
    draws sit on the two clamp ends (N < Ns, below the 50 of kde1d.m:126: the bracket starts at 1e-12 and doubles; t* ~ 1e-9), and a
    type-0 variable.  (At a standard deviation of ~60 some hundred draws land where the doubles next to a bound are coarse, and
    length(unique(data)) falls below the clamp-end rule: 1595 against 1692.)"""
    tr = dict(lb_orig=np.array([-1.0, -np.inf]), ub_orig=np.array([3.0, np.inf]), type=np.array([3, 0]), mu=np.array([0.2, -0.1]),
              delta=np.array([1.3, 0.8]), scale=None, R_mat=None)
    vp = dict(D=2, K=3, mu=np.array([[0.0, 10.0, -10.0], [-0.2, 0.0, 0.3]]), sigma=np.array([2400.0, 2000.0, 1600.0]), w=np.array([0.5, 0.3, 0.2]), trinfo=tr)
    vp["lambda"] = np.array([1.0, 0.01])
    return vp


def make_pair(name):
    """(vp1, vp2, Ns, nkde, nquad, same_block) of a case.  Between them the cases take D in {1, 2, 5, 13, 32} (the padded widths 4,
    8, 16, 32), K in {1, 3, 72}, Ns in {51, 63, 64, 65, 1003, 4097}, nkde in {256, 8192, 16384} and nquad in {2, 1000, 100000}."""
    from tests import _vptools_ref as T

    if name == "empty":            # an empty trinfo; overlapping meshes
        return _gauss(1, 0.0, 1.0), _gauss(1, 0.5, 1.3), 51, 256, 2, False
    if name == "mixed":            # types 0 .. 3 with scale and R_mat
        vp = T.make_case("G")
        return vp, T.sibling(vp), 1003, 8192, 100000, False
    if name == "bounds":           # two posteriors with different bounds
        vp = T.make_vp(2, 3, [3, 1], False, seed=5)
        return vp, _other_bounds(T.sibling(vp)), 63, 256, 1000, False
    if name == "wide13":
        vp = T.make_case("J")
        return vp, T.sibling(vp), 64, 256, 1000, False
    if name == "wide32":
        vp = T.make_case("E", width=2.0)   # (at width 1 two of the 64 columns have three roots in their bracket)
        return vp, T.sibling(vp), 1003, 256, 1000, False
    if name == "pile":             # samples pile on both clamp ends
        vp = make_pile()
        return vp, T.sibling(vp, same_mu=True), 4097, 8192, 1000, False
    if name == "disjoint":         # mtv ~ 1
        return _gauss(1, 0.0, 1.0), _gauss(1, 100.0, 1.0), 1003, 256, 1000, False
    if name == "nested":
        return _gauss(1, 0.0, 1.0), _gauss(1, 0.1, 0.05), 65, 8192, 1000, False
    if name == "identical":        # vp1 == vp2 on one block: the same samples (K = 1: every sample is kept; the permutation of the
        vp = T.make_vp(2, 1, [0, 3], False, seed=7)   # rows is keyed by the seed), two segments of zero length, mtv exactly 0
        return vp, vp, 1003, 256, 1000, True
    if name == "mesh16k":          # the largest mesh: the cosine table takes 128 KB + 8 of LDS
        return _gauss(1, 0.0, 1.0), _gauss(1, 0.5, 1.3), 1003, 16384, 1000, False
    raise KeyError(name)


PAIRS = ("empty", "mixed", "bounds", "wide13", "wide32", "pile", "disjoint", "nested", "identical", "mesh16k")


def make_degenerate():
    """D = 3: in the middle dimension sigma lambda is so small next to the mean that every draw rounds to the mean"""
    vp = dict(D=3, K=1, mu=np.array([[0.0], [1.0], [-0.5]]), sigma=np.array([1.0]), w=np.array([1.0]), trinfo=None)
    vp["lambda"] = np.array([1.0, 1e-30, 0.7])
    return vp

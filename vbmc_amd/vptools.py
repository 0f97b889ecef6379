"""The variational posterior in the caller's own parameter space: vbmc_pdf, vbmc_rnd, vbmc_moments, vbmc_kldiv and vbmc_mtv with the
variable transform of shared/warpvars_vbmc.m on the device (include/vbmc_hip.h: vbmc_vp_pdf, vbmc_vp_rnd, vbmc_vp_moments,
vbmc_vp_kldiv, vbmc_vp_mtv), vbmc_diagnostics over several runs (vbmc_vp_diagnostics: every pair's divergences in one call) and the
data of vbmc_plot's corner plot (vbmc_vp_corner: histograms, pair densities and quantiles of the draws in one call).

``vp["trinfo"]`` is a dict with the reference's field names (lb_orig, ub_orig, type, mu, delta and, optionally, scale and R_mat), or
None / empty for the identity.  Transform types 0 .. 3 are accelerated; anything else raises VbmcUnsupported, on which a caller falls
through to the reference.  The functions keep the reference's argument order; ``seed=`` keys the library's own draws, ``block=``
replays a block written by ``vp_rnd_rng_dump``.  Component indices count from 0.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings

import numpy as np

from . import _lib, mixture
from ._lib import VbmcUnsupported, f64, host_dump, new_args, ptr
from ._pack import U64, Desc as _Desc, i32p, i64p, trinfo_rot as _rot, trinfo_row as _row, trinfo_scale as _scale
from .elbo import default_engine
from .gplite import gplite_sample_device


def warpvars(x, action, trinfo):
    """warpvars_vbmc(x, action, trinfo) for action 'd' (direct, :77-111, :273-279), 'i' (inverse with the clamp, :282-320, :456-460),
    'l' / 'p' (log-Jacobian resp. Jacobian, :463-503, :762-768); transform types 0 .. 3.  Host NumPy."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    act = str(action).lower()[:1]
    if act not in ("d", "i", "l", "p"):
        raise ValueError("warpvars: action %r (d, i, l or p)" % (action,))
    if trinfo is None or len(trinfo) == 0:                        # :47-58
        return x.copy() if act in ("d", "i") else (np.ones(x.shape[0]) if act == "p" else np.zeros(x.shape[0]))
    D = x.shape[1]
    typ = np.asarray(trinfo["type"]).reshape(D).astype(int)
    if np.any((typ < 0) | (typ > 3)):
        raise VbmcUnsupported(-1, "warpvars: transform types 0 .. 3 are supported, got %s" % sorted(set(typ[(typ < 0) | (typ > 3)].tolist())))
    a, b, mu, delta = (_row(trinfo, n, D) for n in ("lb_orig", "ub_orig", "mu", "delta"))
    sc, R = _scale(trinfo, D), _rot(trinfo, D)
    i0, i1, i2, i3 = (typ == t for t in range(4))
    with np.errstate(all="ignore"):
        if act == "d":
            y = x.copy()
            y[:, i0] = (x[:, i0] - mu[i0]) / delta[i0]
            y[:, i1] = np.log(x[:, i1] - a[i1])
            y[:, i2] = np.log(b[i2] - x[:, i2])
            z = (x[:, i3] - a[i3]) / (b[i3] - a[i3])
            y[:, i3] = (np.log(z / (1 - z)) - mu[i3]) / delta[i3]
            if R is not None:
                y = y @ R
            if sc is not None:
                y = y / sc
            return y
        y = x * sc if sc is not None else x.copy()
        if R is not None:
            y = y @ R.T
        if act == "i":
            out = y.copy()
            out[:, i0] = y[:, i0] * delta[i0] + mu[i0]
            out[:, i1] = np.exp(y[:, i1]) + a[i1]
            out[:, i2] = b[i2] - np.exp(y[:, i2])
            out[:, i3] = a[i3] + (b[i3] - a[i3]) * (1.0 / (1.0 + np.exp(-(y[:, i3] * delta[i3] + mu[i3]))))
            lo = np.where(np.isfinite(a), a + np.spacing(np.abs(a)), a)
            hi = np.where(np.isfinite(b), b - np.spacing(np.abs(b)), b)
            return np.minimum(np.maximum(out, lo), hi)
        p = np.zeros_like(y)
        p[:, i0] = np.log(delta[i0])
        p[:, i1 | i2] = y[:, i1 | i2]
        z = y[:, i3] * delta[i3] + mu[i3]
        p[:, i3] = np.log(b[i3] - a[i3]) + (-z + 2 * (-np.log1p(np.exp(-z)))) + np.log(delta[i3])
        if sc is not None:
            p = p + np.log(sc)
        p = np.sum(p, axis=1)
        return p if act == "l" else np.exp(p)


def _engine(engine):
    return default_engine() if engine is None else engine


def _block(block):
    return None if block is None else f64(np.asarray(block, dtype=np.float64).reshape(-1))


def split_size(w, N, balanceflag):
    """M: the number of samples the split of vbmc_rnd.m:57-77 holds before randperm keeps N of them (unbalanced: N)"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    N = int(N)
    if not balanceflag:
        return N
    nf = np.floor(w * N)
    M0 = int(np.sum(nf))
    if N <= M0:
        return M0
    return M0 + int(np.ceil(np.cumsum(w * N - nf)[-1]))


def vp_rnd_rng_dump(seed, N, D, w, balanceflag=False):
    """(B, perm): the block ``seed`` stands for -- B (M, D + 1), row i the slots of sample i (a uniform, then D standard normals) --
    and the permutation perm (N,): output row r is sample perm[r]."""
    w = f64(np.asarray(w, dtype=np.float64).reshape(-1))
    N, D, K = int(N), int(D), w.size
    B = np.zeros((N + K, D + 1), dtype=np.float64)
    perm = np.zeros(N, dtype=np.int64)
    host_dump("vbmc_vp_rnd_rng_dump", seed, N, D, K, 1 if balanceflag else 0, w, B, perm,
              hip_error="vbmc_vp_rnd_rng_dump(N=%d, D=%d, K=%d)" % (N, D, K))
    return B[: split_size(w, N, balanceflag)].copy(), perm


def vbmc_pdf(vp, X, origflag=True, logflag=False, transflag=False, df=np.inf, *, nargout=1, engine=None):
    """[y,dy] = vbmc_pdf(vp,X,origflag,logflag,transflag,df) on the device.  dy (nargout = 2): the Gaussian mixture in the
    transformed space only."""
    engine = _engine(engine)
    ctx = engine.ctx
    d = _Desc(vp)
    X = np.asarray(X, dtype=np.float64)
    X = f64(X.reshape(-1, d.D))
    N = X.shape[0]
    y = np.zeros(N, dtype=np.float64)
    dy = np.zeros((N, d.D), dtype=np.float64, order="F") if nargout > 1 else None
    ctx.check(ctx.lib.vbmc_vp_pdf(ctx.h, d.ref(), N, ptr(X), int(bool(origflag)), int(bool(logflag)), int(bool(transflag)), float(df), ptr(y), ptr(dy)))
    return (y, dy) if nargout > 1 else y


def vbmc_rnd(vp, N, origflag=True, balanceflag=False, df=np.inf, *, seed=0, block=None, nargout=2, engine=None):
    """[X,I] = vbmc_rnd(vp,N,origflag,balanceflag,df), the DEVICE form (mixture.vbmc_rnd is the host draw with a NumPy rng).  Gaussian
    components; 'gp' and a finite df: VbmcUnsupported."""
    engine = _engine(engine)
    ctx = engine.ctx
    d = _Desc(vp)
    N = int(N)
    if N < 1:
        return (np.zeros((0, d.D)), np.zeros(0, dtype=int)) if nargout > 1 else np.zeros((0, d.D))
    bal = 2 if isinstance(balanceflag, str) and balanceflag.lower() == "gp" else int(bool(balanceflag))
    X = np.zeros((N, d.D), dtype=np.float64, order="F")
    I = np.zeros(N, dtype=np.int32)
    B = _block(block)
    ctx.check(ctx.lib.vbmc_vp_rnd(ctx.h, d.ref(), N, int(bool(origflag)), bal, float(df), C.c_uint64(int(seed)), ptr(B), ptr(X),
                                  I.ctypes.data_as(i32p)))
    return (X, I.astype(int)) if nargout > 1 else X


def vbmc_moments(vp, origflag=True, Ns=1e6, *, seed=0, block=None, engine=None):
    """[mubar,Sigma] = vbmc_moments(vp,origflag,Ns), the DEVICE form: the original space by Ns balanced draws on the device (the samples
    never reach memory); the transformed space (origflag = 0) is the analytic host form, mixture.vbmc_moments."""
    if not origflag:
        return mixture.vbmc_moments(vp, False)
    engine = _engine(engine)
    ctx = engine.ctx
    d = _Desc(vp)
    mubar = np.zeros(d.D, dtype=np.float64)
    Sigma = np.zeros((d.D, d.D), dtype=np.float64, order="F")
    B = _block(block)
    ctx.check(ctx.lib.vbmc_vp_moments(ctx.h, d.ref(), int(Ns), C.c_uint64(int(seed)), ptr(B), ptr(mubar), ptr(Sigma)))
    return mubar, np.ascontiguousarray(Sigma)


def mvnkl(mu1, Sigma1, mu2, Sigma2):
    """[kl1,kl2] = mvnkl(Mu1,Sigma1,Mu2,Sigma2) (shared/mvnkl.m)"""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    D = mu1.size
    dmu = mu2 - mu1
    lndet = np.log(np.linalg.det(Sigma2) / np.linalg.det(Sigma1))
    kl1 = 0.5 * (np.trace(np.linalg.solve(Sigma2, Sigma1)) + dmu @ np.linalg.solve(Sigma2, dmu) - D + lndet)
    kl2 = 0.5 * (np.trace(np.linalg.solve(Sigma1, Sigma2)) + dmu @ np.linalg.solve(Sigma1, dmu) - D - lndet)
    return kl1, kl2


def vbmc_kldiv(vp1, vp2, Ns=1e5, gaussflag=False, *, seed=0, block1=None, block2=None, nargout=1, engine=None):
    """[kls,xx1,xx2] = vbmc_kldiv(vp1,vp2,Ns,gaussflag).  The standard divergence runs on the device in one call; direction 2 draws
    with seed + 1.  The Gaussianized one (vbmc_kldiv.m:44-67) is two vbmc_moments and the reference's mvnkl on the host; there vp1 /
    vp2 may be sample matrices."""
    Ns = int(Ns)
    if gaussflag:
        if Ns == 0:
            raise ValueError("vbmc_kldiv: analytical moments are available only for the transformed space")      # :46-49
        mom = []
        for j, v in enumerate((vp1, vp2)):
            if isinstance(v, dict):
                mom.append(vbmc_moments(v, True, Ns, seed=int(seed) + j, block=(block1, block2)[j], engine=engine))
            else:
                v = np.asarray(v, dtype=np.float64)
                mom.append((np.mean(v, axis=0), np.cov(v, rowvar=False).reshape(v.shape[1], v.shape[1])))
        kls = np.maximum(np.array(mvnkl(mom[0][0], mom[0][1], mom[1][0], mom[1][1])), 0.0)
        return (kls, None, None) if nargout > 1 else kls
    if not (isinstance(vp1, dict) and isinstance(vp2, dict)):
        raise ValueError("vbmc_kldiv: unless the KL divergence is Gaussianized, vp1 and vp2 need to be variational posteriors")   # :38-41
    engine = _engine(engine)
    ctx = engine.ctx
    d1, d2 = _Desc(vp1), _Desc(vp2)
    kls = np.zeros(2, dtype=np.float64)
    xx1 = np.zeros((Ns, d1.D), dtype=np.float64, order="F") if nargout > 1 else None
    xx2 = np.zeros((Ns, d1.D), dtype=np.float64, order="F") if nargout > 2 else None
    B1, B2 = _block(block1), _block(block2)
    ctx.check(ctx.lib.vbmc_vp_kldiv(ctx.h, d1.ref(), d2.ref(), Ns, C.c_uint64(int(seed)), ptr(B1), ptr(B2), ptr(kls), ptr(xx1), ptr(xx2)))
    return (kls, xx1, xx2) if nargout > 1 else kls


def vbmc_mtv(vp1, vp2, Ns=1e5, *, seed=0, block1=None, block2=None, nkde=None, nquad=None, nargout=1, stages=False, engine=None):
    """[mtv,xx1,xx2] = vbmc_mtv(vp1,vp2,Ns) on the device in one call: Ns balanced draws of each posterior (vp2 with seed + 1), Botev's
    kde1d on nkde (default 2^13) mesh points per posterior and dimension, 0.5 * integral |p1 - p2| over nquad (default 1e5) points of
    each of the three segments.  Sample matrices in place of a posterior are the reference's business (ValueError).  stages=True
    appends a dict with mesh (2, D, 2: MIN, MAX), counts (2, D, nkde), nuniq (2, D), tstar (2, D) and density (2, D, nkde)."""
    if not (isinstance(vp1, dict) and isinstance(vp2, dict)):
        raise ValueError("vbmc_mtv: vp1 and vp2 need to be variational posteriors (sample matrices are not accelerated)")
    engine = _engine(engine)
    ctx = engine.ctx
    d1, d2 = _Desc(vp1), _Desc(vp2)
    Ns, D = int(Ns), d1.D
    n = 8192 if not nkde else int(nkde)
    a = new_args(_lib.MtvArgs)
    a.nkde, a.nquad, a.Ns, a.seed = int(nkde or 0), int(nquad or 0), Ns, int(seed) & U64
    B1, B2 = _block(block1), _block(block2)
    a.block1, a.block2 = ptr(B1), ptr(B2)
    mtv = np.zeros(D, dtype=np.float64)
    a.mtv = ptr(mtv)
    rows = max(Ns, 0)
    xx1 = np.zeros((rows, D), dtype=np.float64, order="F") if nargout > 1 else None
    xx2 = np.zeros((rows, D), dtype=np.float64, order="F") if nargout > 2 else None
    a.xx1, a.xx2 = ptr(xx1), ptr(xx2)
    st = None
    if stages and 256 <= n <= 16384:
        st = {"mesh": np.zeros((2, D, 2)), "counts": np.zeros((2, D, n), dtype=np.int32), "nuniq": np.zeros((2, D), dtype=np.int64),
              "tstar": np.zeros((2, D)), "density": np.zeros((2, D, n))}
        a.mesh, a.tstar, a.density = ptr(st["mesh"]), ptr(st["tstar"]), ptr(st["density"])
        a.counts = st["counts"].ctypes.data_as(i32p)
        a.nuniq = st["nuniq"].ctypes.data_as(i64p)
    ctx.check(ctx.lib.vbmc_vp_mtv(ctx.h, d1.ref(), d2.ref(), C.byref(a)))
    out = (mtv, xx1, xx2)[: max(1, min(int(nargout), 3))]
    if stages:
        out = out + (st,)
    return out if len(out) > 1 else out[0]


def _corner(ctx, desc, X, Ns, D, seed, block, origflag, balanceflag, bounds, res, nbins, p, stages):
    """One vbmc_vp_corner call; the arrays come back in NumPy's order (see vbmc_plot_data)"""
    n = 64 if not res else int(res)
    nb = 40 if not nbins else int(nbins)
    p = f64(np.asarray(() if p is None else p, dtype=np.float64).reshape(-1))
    P = D * (D - 1) // 2
    a = new_args(_lib.CornerArgs)
    a.D, a.res, a.nbins, a.nq, a.origflag, a.balanceflag = D, int(res or 0), int(nbins or 0), p.size, int(bool(origflag)), int(balanceflag)
    a.Ns, a.seed = Ns, int(seed) & U64
    B = _block(block)
    Xin = None if X is None else f64(X)
    b = None if bounds is None else np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(D, 2))
    a.block, a.X_in, a.bounds, a.p = ptr(B), ptr(Xin), ptr(b), ptr(p) if p.size else None
    rows, sq = max(Ns, 0), (n if n in (16, 32, 64) else 0)
    out = {"xx": np.zeros((rows, D), order="F"), "bounds": np.zeros((D, 2)), "hist": np.zeros((D, max(min(nb, 1024), 0)), dtype=np.int32),
           "quant": np.zeros((D, min(p.size, 16))), "density": np.zeros((P, sq, sq)), "bandwidth": np.zeros((P, 2))}
    a.xx, a.bounds_out, a.quant, a.density, a.bandwidth = (ptr(out[k]) for k in ("xx", "bounds", "quant", "density", "bandwidth"))
    a.hist = out["hist"].ctypes.data_as(i32p)
    if stages:
        out.update(tstar=np.zeros(P), counts2=np.zeros((P, sq, sq), dtype=np.int32))
        a.tstar, a.counts2 = ptr(out["tstar"]), out["counts2"].ctypes.data_as(i32p)
    ctx.check(ctx.lib.vbmc_vp_corner(ctx.h, None if desc is None else desc.ref(), C.byref(a)))
    # the library's res x res x P is column-major: [pp][column][row] in NumPy's order
    out["density"] = np.ascontiguousarray(out["density"].transpose(0, 2, 1))
    if stages:
        out["counts2"] = np.ascontiguousarray(out["counts2"].transpose(0, 2, 1))
    out["pairs"] = [(d1, d2) for d1 in range(D - 1) for d2 in range(d1 + 1, D)]
    out["p"], out["res"], out["Ns"] = p.copy(), n, Ns
    return out


def vbmc_plot_data(vp, Ns=1e5, *, seed=0, block=None, origflag=True, balanceflag=0, bounds=None, res=64, nbins=40, p=(0.5,), stages=False,
                   engine=None):
    """What vbmc_plot(vp) (vbmc_plot.m:12-15; balanceflag=1: private/vbmc_iterplot.m:21, :47) hands to utils/cornerplot.m and what that
    computes from it, on the device in one call (vbmc_vp_corner): Ns draws of the posterior -- vbmc_rnd's rows for ``seed`` --, a
    histogram of nbins equal bins per dimension between its bounds, kde2d on res x res (16, 32 or 64) for every pair of dimensions,
    and the quantiles of utils/quantile1.m at the probabilities ``p``.

    Returns a dict: xx (Ns, D), bounds (D, 2: given, or each column's min and max), hist (D, nbins) counts (the probability is
    hist / Ns), quant (D, len(p)), pairs (the (d1, d2) of each pair in cornerplot's order), density (P, res, res: density[pp][i, j] at
    (d2 mesh point i, d1 mesh point j), as kde2d returns it and contour(X, Y, density) takes it), bandwidth (P, 2); stages=True adds
    tstar (P) and counts2 (P, res, res: [pp][d1 bin, d2 bin]).  The mesh of dimension d is
    ``np.linspace(bounds[d, 0], bounds[d, 1], res)``.  A sample outside given bounds is dropped from the counts and still counts in N,
    as in kde2d.  Raises VbmcUnsupported where a pair reaches kde2d's fminbnd branch, for res above 64 and for what vbmc_rnd refuses:
    there a caller falls through to the reference's plot.  A departure: MATLAB's histogram(x, 40) picks its own "nice" edges."""
    if not isinstance(vp, dict):
        raise ValueError("vbmc_plot_data: vp needs to be a variational posterior (cornerplot_data takes a sample matrix)")
    engine = _engine(engine)
    d = _Desc(vp)
    return _corner(engine.ctx, d, None, int(Ns), d.D, seed, block, origflag, balanceflag, bounds, res, nbins, p, stages)


def cornerplot_data(X, bounds=None, *, res=64, nbins=40, p=(0.5,), stages=False, engine=None):
    """vbmc_plot_data for a given sample matrix X (Ns, D): the numbers of cornerplot(X, names, truths, bounds).  An entry that is not
    finite is a ValueError (VBMC_ERR_INVALID)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("cornerplot_data: X must be a matrix of samples, one per row")
    engine = _engine(engine)
    return _corner(engine.ctx, None, X, X.shape[0], X.shape[1], 0, None, True, 0, bounds, res, nbins, p, stages)


def vbmc_mode(vp, nmax=20, origflag=True, *, nargout=1, details=False, max_iter=0, tol_grad=1e-6, engine=None):
    """[x,vp] = vbmc_mode(vp,nmax,origflag) on the device in one call (vbmc_vp_mode): the mode of the variational posterior, in the
    original space (origflag, the default) or the transformed one.  With origflag a stored ``vp["mode"]`` is returned without a device
    (vbmc_mode.m:18-19) and nargout=2 returns a copy of ``vp`` with ``mode`` stored (:53-55).  details=True appends a dict with fval,
    idx and per start start_comp, f0, us, xs, fs, iters, nfev and stop (the names of _lib.MODE_STOP).

    Intentional divergences from the reference (include/vbmc_hip.h has the whole statement): the optimiser is the library's BFGS on
    the smooth objective in the transformed space, not fmincon in the box; with origflag the starts are ranked by the objective at
    the starts themselves (:24 evaluates the original-space density at transformed-space coordinates); the answer is kept eps, not
    sqrt(eps), from the bounds; a start whose density underflows is still optimised."""
    origflag = bool(origflag)
    stored = vp.get("mode") if origflag else None
    if stored is not None and np.size(stored) > 0 and not details:
        x = np.array(stored, dtype=np.float64).reshape(-1)
        return (x, vp) if nargout > 1 else x
    engine = _engine(engine)
    ctx = engine.ctx
    d = _Desc(vp)
    nmax = _mode_nmax(nmax)
    S = min(nmax, d.K)
    a = new_args(_lib.ModeArgs)
    a.nmax, a.origflag, a.max_iter, a.tol_grad = nmax, int(origflag), int(max_iter), float(tol_grad)
    x, fval, idx, S_out = np.zeros(d.D), C.c_double(), C.c_int32(), C.c_int32()
    a.x, a.fval, a.idx, a.S_out = ptr(x), C.pointer(fval), C.pointer(idx), C.pointer(S_out)
    out = None
    if details:
        out = {"start_comp": np.zeros(S, dtype=np.int32), "f0": np.zeros(S), "us": np.zeros((S, d.D), order="F"), "xs": np.zeros((S, d.D), order="F"),
               "fs": np.zeros(S), "iters": np.zeros(S, dtype=np.int32), "nfev": np.zeros(S, dtype=np.int32), "stop": np.zeros(S, dtype=np.int32)}
        for k, v in out.items():
            setattr(a, k, v.ctypes.data_as(i32p) if v.dtype == np.int32 else ptr(v))
    ctx.check(ctx.lib.vbmc_vp_mode(ctx.h, d.ref(), C.byref(a)))
    res = (x,)
    if nargout > 1:
        vp2 = dict(vp)
        if origflag:
            vp2["mode"] = x.copy()
        res = res + (vp2,)
    if details:
        out = {k: np.ascontiguousarray(v) for k, v in out.items()}
        out.update(fval=float(fval.value), idx=int(idx.value), S=int(S_out.value))
        res = res + (out,)
    return res if len(res) > 1 else res[0]


def _mode_nmax(nmax):
    nmax = 20 if nmax is None else int(nmax)
    return 20 if nmax <= 0 else nmax


def vp_diagnostics(vp_array, Ns=1e5, *, seed=0, nkde=None, nquad=None, stages=False, draws=False, outputs=("kl_mat", "mtv", "maxmtv_mat"),
                   engine=None):
    """The pair loop of vbmc_diagnostics.m:116-127 on the device in one call (vbmc_vp_diagnostics).  Run i draws once, with seed + i.
    Returns a dict: kl_mat (R, R) with kl_mat[i, j] = KL(run i || run j), mtv (R, R, D), maxmtv_mat (R, R) (the maximum over the
    dimensions that are not NaN); stages=True adds mesh (R, D, 2), counts (R, D, nkde), nuniq (R, D), tstar (R, D) and density
    (R, D, nkde); draws=True adds xx (R, Ns, D).  ``outputs`` names the matrices wanted: the library skips the cross densities
    without kl_mat and the integrals without mtv and maxmtv_mat."""
    engine = _engine(engine)
    ctx = engine.ctx
    descs = [_Desc(v) for v in vp_array]
    R, D, Ns = len(descs), descs[0].D if descs else 0, int(Ns)
    n = 8192 if not nkde else int(nkde)
    a = new_args(_lib.DiagArgs)
    a.nkde, a.nquad, a.Ns, a.seed = int(nkde or 0), int(nquad or 0), Ns, int(seed) & U64
    out = {"kl_mat": np.zeros((R, R), order="F"), "mtv": np.zeros((R, R, D)), "maxmtv_mat": np.zeros((R, R), order="F")}
    for k in ("kl_mat", "mtv", "maxmtv_mat"):
        if k in outputs:
            setattr(a, k, ptr(out[k]))
        else:
            del out[k]
    if stages and 256 <= n <= 16384:
        out.update(mesh=np.zeros((R, D, 2)), counts=np.zeros((R, D, n), dtype=np.int32), nuniq=np.zeros((R, D), dtype=np.int64),
                   tstar=np.zeros((R, D)), density=np.zeros((R, D, n)))
        a.mesh, a.tstar, a.density = ptr(out["mesh"]), ptr(out["tstar"]), ptr(out["density"])
        a.counts = out["counts"].ctypes.data_as(i32p)
        a.nuniq = out["nuniq"].ctypes.data_as(i64p)
    if draws:
        xx = np.zeros((R, D, max(Ns, 0)))                       # run i, column d, row r: the ABI's Ns x D x R column-major
        a.xx = ptr(xx)
    arr = (C.POINTER(_lib.VpDesc) * max(R, 1))(*[C.pointer(d.d) for d in descs])
    ctx.check(ctx.lib.vbmc_vp_diagnostics(ctx.h, R, arr, C.byref(a)))
    for k in ("kl_mat", "maxmtv_mat"):
        if k in out:
            out[k] = np.ascontiguousarray(out[k])
    if draws:
        out["xx"] = np.ascontiguousarray(xx.transpose(0, 2, 1))
    return out


_DIAG_MSG = {1: "Diagnostic test PASSED.",
             0: "Diagnostic test FAILED: only one run has converged, so there is nothing to compare it with.",
             -1: "Diagnostic test FAILED: too few runs agree with the best posterior (symmetrized KL divergence or largest marginal total variation).",
             -2: "Diagnostic test FAILED: too few runs agree with the best ELBO.",
             -3: "Diagnostic test FAILED: no run has converged."}


def diagnostics_decision(elbo, elbo_sd, stable, kl_mat, maxmtv_mat, beta_lcb=3, elbo_thresh=1, sKL_thresh=1, maxmtv_thresh=0.2):
    """The decision of vbmc_diagnostics.m:58-114, :129-222 as a function of the runs' statistics and the two distance matrices (host
    only, no device).  Returns a dict with exitflag, idx_best (from 0; None when the best run is not stable), the index best_run the
    comparisons used, elcbo, sKL_best, maxmtv_best, the three boolean rows elbo_ok / sKL_ok / maxmtv_ok (None for one run), msg and
    the list of warnings.

    The best run is the first maximum of elbo - beta_lcb elbo_sd among the converged runs (among all runs when none has converged); a
    NaN there is skipped as MATLAB's max skips it.  A run agrees when |elbo - elbo_best| < elbo_thresh, resp. its symmetrized KL
    divergence to the best run < sKL_thresh, resp. its largest marginal total variation to it < maxmtv_thresh (a NaN never agrees;
    the best run always agrees with itself); each of the three counts has to reach max(Nruns / 3, 2)."""
    elbo = np.asarray(elbo, dtype=np.float64).reshape(-1)
    elbo_sd = np.asarray(elbo_sd, dtype=np.float64).reshape(-1)
    stable = np.asarray(stable).reshape(-1).astype(bool)
    R = elbo.size
    kl_mat = np.asarray(kl_mat, dtype=np.float64).reshape(R, R)
    maxmtv_mat = np.asarray(maxmtv_mat, dtype=np.float64).reshape(R, R)
    notes = []
    exitflag = math.inf
    if R == 1:
        notes.append("vbmc_diagnostics needs the posteriors of several runs; a single run cannot be compared with anything.")
    active = stable.copy()
    nok = int(np.sum(stable))
    if nok == 0:
        notes.append("No run has converged; the comparisons use a solution that may be unstable.")
        active[:] = True
        exitflag = -3
    elif nok == 1:
        notes.append("Only one run has converged; perform more runs.")
        exitflag = 0
    elcbo = elbo - beta_lcb * elbo_sd
    eff = np.where(active, elcbo, -np.inf)
    cand = np.flatnonzero(~np.isnan(eff))
    best = int(cand[np.argmax(eff[cand])]) if cand.size else 0        # the first maximum; NaN skipped; all NaN: the first run
    sKL_best = 0.5 * (kl_mat[:, best] + kl_mat[best, :])
    maxmtv_best = maxmtv_mat[best, :].copy()
    oks = {"elbo_ok": None, "sKL_ok": None, "maxmtv_ok": None}
    if R > 1:
        need = max(R * (1.0 / 3.0), 2)
        with np.errstate(invalid="ignore"):
            oks["elbo_ok"] = np.abs(elbo[best] - elbo) < elbo_thresh
            oks["sKL_ok"] = sKL_best < sKL_thresh
            oks["maxmtv_ok"] = maxmtv_best < maxmtv_thresh
        for key, flag, what in (("elbo_ok", -2, "the best ELBO"), ("sKL_ok", -1, "the best posterior (symmetrized KL divergence)"),
                                ("maxmtv_ok", -1, "the best posterior (largest marginal total variation)")):
            if np.sum(oks[key]) < need:
                notes.append("Too few runs agree with %s." % what)
                exitflag = min(exitflag, flag)
    if math.isinf(exitflag):
        exitflag = 1
    exitflag = int(exitflag)
    return dict(exitflag=exitflag, idx_best=best if stable[best] else None, best_run=best, elcbo=elcbo, sKL_best=sKL_best,
                maxmtv_best=maxmtv_best, msg=_DIAG_MSG[exitflag], warnings=notes, **oks)


def vbmc_diagnostics(vp_array, beta_lcb=3, elbo_thresh=1, sKL_thresh=1, maxmtv_thresh=0.2, *, Ns=1e5, seed=0, nkde=None, nquad=None,
                     stages=False, verbose=True, engine=None):
    """[exitflag,best,idx_best,stats] = vbmc_diagnostics(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh): the convergence
    diagnostics over several VBMC runs, every pair's KL divergences and marginal total variations in ONE device call.  Each vp dict
    carries ``stats = {elbo, elbo_sd, stable}``.  Exit flags: 1 passed; 0 only one run converged; -1 too few runs agree with the best
    posterior; -2 too few agree with the best ELBO; -3 no run converged.  ``best`` = {vp, elbo, elbo_sd} and ``idx_best`` (from 0) are
    None when the best run is not stable.  ``stats`` has the reference's fields (vbmc_diagnostics.m:226-239); stages=True adds the
    device call's stage outputs under ``stats["stages"]``.  One run needs no device call: the matrices are zero and a warning is given.

    Intentional divergences from the reference:
      * run i draws once (seed + i) and meets every other run on those draws; the reference draws afresh for every pair.
      * vbmc_diagnostics.m:53-56 test ``nargin`` one too high, so there the last argument a caller gives is overwritten by its default.
        Here, as the help text (:30-49) says, an argument that is given is used.
    Kept from the reference: maxmtv_mat is the maximum over the dimensions that are not NaN (MATLAB's max at :124 skips NaN)."""
    vps = list(vp_array)
    R = len(vps)
    if R < 1:
        raise ValueError("vbmc_diagnostics: vp_array is empty")
    D = int(vps[0]["D"])
    elbo = np.array([float(v["stats"]["elbo"]) for v in vps])
    elbo_sd = np.array([float(v["stats"]["elbo_sd"]) for v in vps])
    stable = np.array([bool(v["stats"]["stable"]) for v in vps])
    dev = None
    if R > 1:
        dev = vp_diagnostics(vps, Ns, seed=seed, nkde=nkde, nquad=nquad, stages=stages, engine=engine)
        kl_mat, maxmtv_mat = dev["kl_mat"], dev["maxmtv_mat"]
    else:
        kl_mat, maxmtv_mat = np.zeros((1, 1)), np.zeros((1, 1))
    dec = diagnostics_decision(elbo, elbo_sd, stable, kl_mat, maxmtv_mat, beta_lcb, elbo_thresh, sKL_thresh, maxmtv_thresh)
    notes = list(dec["warnings"])
    rec = max(2, int(math.ceil(math.log2(D)))) if D > 1 else 2
    if R < rec:
        notes.append("For a problem in D = %d dimensions at least %d runs are recommended." % (D, rec))
    for m in notes:
        warnings.warn(m, stacklevel=2)
    if verbose:
        print("%d of %d runs have converged." % (int(np.sum(stable)), R))
        print(" run         elbo     elbo_sd        elcbo  converged    sKL[best]  maxMTV[best]")
        for i in range(R):
            print("%4d %12.2f %11.2f %12.2f %10s %12.2f %13.2f %s" % (i, elbo[i], elbo_sd[i], dec["elcbo"][i], "yes" if stable[i] else "no",
                                                                     dec["sKL_best"][i], dec["maxmtv_best"][i], "best" if i == dec["best_run"] else ""))
        for key, what, thr in (("elbo_ok", "the best ELBO", elbo_thresh), ("sKL_ok", "the best posterior in symmetrized KL", sKL_thresh),
                               ("maxmtv_ok", "the best posterior in largest marginal total variation", maxmtv_thresh)):
            if dec[key] is not None:
                print("%d of %d runs agree with %s (below %g)." % (int(np.sum(dec[key])), R, what, thr))
        print(dec["msg"])
    idx_best = dec["idx_best"]
    best = None if idx_best is None else {"vp": vps[idx_best], "elbo": float(elbo[idx_best]), "elbo_sd": float(elbo_sd[idx_best])}
    stats = dict(beta_lcb=beta_lcb, elbo_thresh=elbo_thresh, sKL_thresh=sKL_thresh, maxmtv_thresh=maxmtv_thresh, elbo=elbo, elbo_sd=elbo_sd,
                 elcbo=dec["elcbo"], idx_best=idx_best, sKL_best=dec["sKL_best"], maxmtv_best=dec["maxmtv_best"], kl_mat=kl_mat,
                 maxmtv_mat=maxmtv_mat, exitflag=dec["exitflag"], msg=dec["msg"])
    if dev is not None:
        stats["mtv"] = dev["mtv"]
        if stages:
            stats["stages"] = {k: dev[k] for k in ("mesh", "counts", "nuniq", "tstar", "density") if k in dev}
    return dec["exitflag"], best, idx_best, stats


def _training_noise(gp):
    """sn2new of gpsample_vbmc.m:17-28: gplite_noisefun (gplite_noisefun.m:176-210) at the training inputs, the mean over hyper-samples"""
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    nf = tuple(int(v) for v in gp["noisefun"]) + (0,) * (3 - len(gp["noisefun"]))
    y = np.asarray(gp["y"], dtype=np.float64).reshape(-1)
    s2 = np.asarray(gp["s2"], dtype=np.float64).reshape(-1)
    Ncov = int(gp.get("Ncov", D + 1))
    acc = np.zeros(N)
    for post in gp["post"]:
        hn = np.asarray(post["hyp"], dtype=np.float64).reshape(-1)[Ncov:]
        idx = 0
        sn2 = np.full(N, np.finfo(np.float64).eps)
        if nf[0] == 1:
            sn2 = np.full(N, np.exp(2 * hn[idx]))
            idx += 1
        if nf[1] == 1:
            sn2 = sn2 + s2
        elif nf[1] == 2:
            sn2 = sn2 + np.exp(hn[idx]) * s2
            idx += 1
        if nf[2] == 1:
            sn2 = sn2 + np.exp(2 * hn[idx + 1]) * np.maximum(0.0, hn[idx] - y) ** 2
        acc = acc + sn2
    return acc / len(gp["post"])


def gpsample_noise_setup(gp):
    """The host set-up of the noise estimate (gpsample_vbmc.m:8-28): None for a GP without s2, or a dict with gplengthscale (the
    geometric mean of the length scales over hyper-samples), X_rescaled and sn2new."""
    s2 = gp.get("s2")
    if s2 is None or np.size(s2) == 0:
        return None
    X = np.asarray(gp["X"], dtype=np.float64)
    D = X.shape[1]
    ln_ell = np.stack([np.asarray(p["hyp"], dtype=np.float64).reshape(-1)[:D] for p in gp["post"]], axis=1)
    gl = np.exp(np.mean(ln_ell, axis=1))
    return {"gplengthscale": gl, "X_rescaled": X / gl[None, :], "sn2new": _training_noise(gp)}


def gpsample_vbmc(vp, gp, Ns, origflag=True, *, E=1, seed=0, Nnn=0, bounds=None, thin=1, burnin=None, spec=0, chunk=0, uniforms=None,
                  nargout=1, engine=None):
    """X = gpsample_vbmc(vp,gp,Ns,origflag) on the device in one call: the noise estimate over Nnn (0: 20000) draws of ``vp`` where the
    GP carries s2 (VarThresh = max(1, sn2_avg), :30-38), W = 2 (D + 1) starting walkers per ensemble drawn from ``vp`` (:41), the
    'parallel' chain of gplite_sample on its default box, and the way back to the original space (:43-45).  E > 1 runs that many
    independent ensembles, each with its own burn-in.  nargout=2 adds the dict of ``gplite.gplite_sample_device``."""
    X = np.asarray(gp["X"], dtype=np.float64)
    D = X.shape[1]
    if bounds is None or np.size(bounds) == 0:                                   # gplite_sample.m:16-20
        diam = np.max(X, axis=0) - np.min(X, axis=0)
        LB, UB = np.min(X, axis=0) - 10 * diam, np.max(X, axis=0) + 10 * diam
    else:
        bounds = np.asarray(bounds, dtype=np.float64).reshape(2, D)
        LB, UB = bounds[0], bounds[1]
    noise = gpsample_noise_setup(gp)
    if noise is not None:
        noise["Nnn"] = int(Nnn)
    r = gplite_sample_device(gp, Ns, LB, UB, vp=vp, E=E, thin=thin, burnin=burnin, VarThresh=1.0, noise=noise, origflag=origflag, spec=spec,
                             chunk=chunk, seed=seed, uniforms=uniforms, outputs=("X", "Xt", "logp") if nargout > 1 else ("X",), engine=_engine(engine))
    return (r["X"], r) if nargout > 1 else r["X"]

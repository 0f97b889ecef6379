"""The variational posterior in the caller's own parameter space: vbmc_pdf, vbmc_rnd, vbmc_moments, vbmc_kldiv and vbmc_mtv with the
variable transform of shared/warpvars_vbmc.m on the device (include/vbmc_hip.h: vbmc_vp_pdf, vbmc_vp_rnd, vbmc_vp_moments,
vbmc_vp_kldiv, vbmc_vp_mtv).

``vp["trinfo"]`` is a dict with the reference's field names (lb_orig, ub_orig, type, mu, delta and, optionally, scale and R_mat), or
None / empty for the identity.  Transform types 0 .. 3 are accelerated; anything else raises VbmcUnsupported, on which a caller falls
through to the reference.  The functions keep the reference's argument order; ``seed=`` keys the library's own draws, ``block=``
replays a block written by ``vp_rnd_rng_dump``.  Component indices count from 0.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import VbmcUnsupported, f64, ptr


def _trinfo(vp):
    tr = vp.get("trinfo") if isinstance(vp, dict) else None
    if tr is None or len(tr) == 0:
        return None
    return tr


def _row(tr, name, D):
    return np.asarray(tr[name], dtype=np.float64).reshape(D)


def _scale(tr, D):
    """warpvars_vbmc.m:66-69: the scale row counts only where it differs from one"""
    sc = tr.get("scale")
    if sc is None or np.size(sc) == 0:
        return None
    sc = np.asarray(sc, dtype=np.float64).reshape(D)
    return sc if np.any(sc != 1) else None


def _rot(tr, D):
    R = tr.get("R_mat")
    if R is None or np.size(R) == 0:
        return None
    return np.asarray(R, dtype=np.float64).reshape(D, D)


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


class _Desc:
    """A vbmc_vp_desc and the arrays it points at"""

    def __init__(self, vp):
        D, K = int(vp["D"]), int(vp["K"])
        self.D, self.K = D, K
        self.keep = [f64(np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)), f64(np.asarray(vp["sigma"], dtype=np.float64).reshape(K)),
                     f64(np.asarray(vp["lambda"], dtype=np.float64).reshape(D)), f64(np.asarray(vp["w"], dtype=np.float64).reshape(K))]
        d = _lib.VpDesc()
        d.struct_size = C.sizeof(_lib.VpDesc)
        d.D, d.K = D, K
        d.mu, d.sigma, d.w = ptr(self.keep[0]), ptr(self.keep[1]), ptr(self.keep[3])
        setattr(d, "lambda", ptr(self.keep[2]))
        tr = _trinfo(vp)
        if tr is not None:
            typ = np.ascontiguousarray(np.asarray(tr["type"]).reshape(D).astype(np.int32))
            rows = [f64(_row(tr, n, D)) for n in ("lb_orig", "ub_orig", "mu", "delta")]
            sc, R = _scale(tr, D), _rot(tr, D)
            self.keep += [typ] + rows
            d.type = typ.ctypes.data_as(C.POINTER(C.c_int32))
            d.lb, d.ub, d.tmu, d.tdelta = (ptr(r) for r in rows)
            if sc is not None:
                sc = f64(sc)
                self.keep.append(sc)
                d.scale = ptr(sc)
            if R is not None:
                R = f64(R)
                self.keep.append(R)
                d.R = ptr(R)
        self.d = d

    def ref(self):
        return C.byref(self.d)


def _engine(engine):
    if engine is None:
        from .elbo import default_engine
        engine = default_engine()
    return engine


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
    lib = _lib.load()
    w = f64(np.asarray(w, dtype=np.float64).reshape(-1))
    N, D, K = int(N), int(D), w.size
    B = np.zeros((N + K, D + 1), dtype=np.float64)
    perm = np.zeros(N, dtype=np.int64)
    st = lib.vbmc_vp_rnd_rng_dump(C.c_uint64(int(seed)), N, D, K, 1 if balanceflag else 0, ptr(w), ptr(B), perm.ctypes.data_as(C.POINTER(C.c_int64)))
    if st != _lib.VBMC_OK:
        raise _lib.VbmcHipError(st, "vbmc_vp_rnd_rng_dump(N=%d, D=%d, K=%d)" % (N, D, K))
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
    """[X,I] = vbmc_rnd(vp,N,origflag,balanceflag,df) on the device (Gaussian components; 'gp' and a finite df: VbmcUnsupported)"""
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
                                  I.ctypes.data_as(C.POINTER(C.c_int32))))
    return (X, I.astype(int)) if nargout > 1 else X


def vbmc_moments(vp, origflag=True, Ns=1e6, *, seed=0, block=None, engine=None):
    """[mubar,Sigma] = vbmc_moments(vp,origflag,Ns): the original space by Ns balanced draws on the device (the samples never reach
    memory); the transformed space (origflag = 0) is the analytic host form."""
    if not origflag:
        from .acq import vbmc_moments as _analytic
        return _analytic(vp, False)
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
    a = _lib.MtvArgs()
    a.struct_size = C.sizeof(_lib.MtvArgs)
    a.nkde, a.nquad, a.Ns, a.seed = int(nkde or 0), int(nquad or 0), Ns, int(seed) & (2 ** 64 - 1)
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
        a.counts = st["counts"].ctypes.data_as(C.POINTER(C.c_int32))
        a.nuniq = st["nuniq"].ctypes.data_as(C.POINTER(C.c_int64))
    ctx.check(ctx.lib.vbmc_vp_mtv(ctx.h, d1.ref(), d2.ref(), C.byref(a)))
    out = (mtv, xx1, xx2)[: max(1, min(int(nargout), 3))]
    if stages:
        out = out + (st,)
    return out if len(out) > 1 else out[0]


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
    from .gplite import gplite_sample_device

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

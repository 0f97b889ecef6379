"""Packers of the argument groups that several entry points of include/vbmc_hip.h share: each group is laid out here once.

A packer fills the fields of the argument struct its caller passes (``a``; None where the entry point takes plain arguments) and
returns the arrays those fields point at: the caller keeps them referenced until the library call has returned.  ``who`` is the
caller's name, the prefix of every message.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import VBMC_ERR_UNSUPPORTED, VbmcUnsupported, VpDesc, f64, new_args, ptr

U64 = 2 ** 64 - 1
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def row(v, n, default=None):
    """``v`` as n contiguous doubles, a single value repeated; ``default`` stands in for None or an empty ``v``"""
    if default is not None and (v is None or np.size(v) == 0):
        v = default
    return f64(np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (n,)).copy())


def box(LB, UB, n, open_ended=False):
    """(lb, ub), n doubles each.  ``open_ended``: a missing or empty bound is -inf resp. +inf (the two training calls)."""
    return row(LB, n, -np.inf if open_ended else None), row(UB, n, np.inf if open_ended else None)


def mixture(vp, a=None, prefix="vp_", D=None):
    """(mu (D, K), sigma (K), lambda (D), w (K)) of the variational posterior; fills ``a.<prefix>mu`` .. ``a.<prefix>w``"""
    D, K = int(vp["D"] if D is None else D), int(vp["K"])
    arrs = tuple(f64(np.asarray(vp[name], dtype=np.float64).reshape(shape))
                 for name, shape in (("mu", (D, K)), ("sigma", K), ("lambda", D), ("w", K)))
    if a is not None:
        for name, arr in zip(("mu", "sigma", "lambda", "w"), arrs):
            setattr(a, prefix + name, ptr(arr))
    return arrs


def delta_row(vp, D):
    """vp.delta as D doubles (gplite_quad's bsxfun admits a scalar, gplite_quad.m:70), None where the posterior has none"""
    delta = vp.get("delta")
    return None if delta is None or np.size(delta) == 0 else row(delta, D)


def training_block(a, gp, who):
    """N, D, meanfun, noisefun, X, y, s2 of the two GP-training calls, and their refusal of what the objective layer does not cover"""
    if gp.get("intmeanfun", 0) or gp.get("outwarpfun") is not None or int(np.atleast_1d(gp.get("covfun", 1))[0]) != 1:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "%s: integrated mean / output warping / non-SE covariance are not accelerated" % who)
    X = f64(gp["X"])
    y = f64(np.asarray(gp["y"], dtype=np.float64).reshape(-1))
    s2 = gp.get("s2")
    s2 = None if s2 is None or np.size(s2) == 0 else f64(np.asarray(s2, dtype=np.float64).reshape(-1))
    (a.N, a.D), a.meanfun = X.shape, int(gp["meanfun"])
    a.noisefun[:] = [int(v) for v in (list(gp["noisefun"]) + [0, 0, 0])[:3]]
    a.X, a.y, a.s2 = ptr(X), ptr(y), ptr(s2)
    return X, y, s2


def hyper_prior(a, hprior, Nhyp, who, needs_mu=False):
    """prior_mu / prior_sigma / prior_df, one entry per hyper-parameter.  The two callers differ in one point, kept as it was:
    gplite_train_optimize (``needs_mu``) takes an ``hprior`` without ``mu`` for no prior at all, slicesamplebnd_gp requires the field."""
    if hprior is None or (needs_mu and (hprior.get("mu") is None or np.size(hprior.get("mu")) == 0)):
        return ()
    mu = f64(np.asarray(hprior["mu"], dtype=np.float64).reshape(-1))
    sg = f64(np.asarray(hprior["sigma"], dtype=np.float64).reshape(-1))
    df = hprior.get("df")
    df = None if df is None or np.size(df) == 0 else f64(np.asarray(df, dtype=np.float64).reshape(-1))
    if mu.size != Nhyp or sg.size != Nhyp or (df is not None and df.size != Nhyp):
        raise ValueError("%s: hprior.mu / sigma / df need one entry per hyper-parameter" % who)
    a.prior_mu, a.prior_sigma, a.prior_df = ptr(mu), ptr(sg), ptr(df)
    return mu, sg, df


def sampler_opts(a, W, N, thin, burnin, spec, max_steps, max_shrink, chunk, seed):
    """The options of the ensemble slice sampler on the device (vbmc_is_sample_args, vbmc_is_setup_args, vbmc_gs_args): W walkers,
    N samples (the field Nm, or Ns), burnin None for the library's default, the library's generator keyed by ``seed``."""
    a.W, a.thin, a.burnin, a.spec = int(W), int(thin), -1 if burnin is None else int(burnin), int(spec)
    setattr(a, "Nm" if hasattr(a, "Nm") else "Ns", int(N))
    a.max_steps, a.max_shrink, a.chunk = int(max_steps), int(max_shrink), int(chunk)
    a.rng_mode, a.seed = 0, int(seed) & U64


def sampler_uniforms(a, uniforms, H, E, who, axis="S"):
    """The caller's uniforms 64 x H x E x Mmax in place of the generator's (Mmax, U; the caller sets rng_mode, which the set-up
    shares with its Step 1 block)"""
    U = f64(np.asarray(uniforms, dtype=np.float64))
    if U.ndim != 4 or U.shape[:3] != (64, H, E):
        raise ValueError("%s: uniforms must be 64 x H x %s x Mmax = 64 x %d x %d x Mmax" % (who, axis, H, E))
    a.Mmax, a.U = U.shape[3], ptr(U)
    return U


def counters(a):
    """Point funccount / performed / rounds[2] at fresh counters; returns the reader of their values after the call"""
    fc, pf, rounds = C.c_int64(), C.c_int64(), (C.c_int64 * 2)()
    a.funccount, a.performed, a.rounds = C.pointer(fc), C.pointer(pf), C.cast(rounds, i64p)
    return lambda: {"funccount": int(fc.value), "performed": int(pf.value), "rounds": int(rounds[0]), "behind": int(rounds[1])}


def nn_noise(a, gplengthscale, X_rescaled, sn2new, N, D):
    """(gplengthscale (D), X_rescaled (N, D), sn2new (N)): the nearest-neighbour noise estimate's inputs; a None stays NULL"""
    gl = None if gplengthscale is None else f64(np.asarray(gplengthscale, dtype=np.float64).reshape(D))
    xr = None if X_rescaled is None else f64(np.asarray(X_rescaled, dtype=np.float64).reshape(N, D))
    sn = None if sn2new is None else f64(np.asarray(sn2new, dtype=np.float64).reshape(N))
    if a is not None:
        a.gplengthscale, a.X_rescaled, a.sn2new = ptr(gl), ptr(xr), ptr(sn)
    return gl, xr, sn


def trinfo_of(vp):
    tr = vp.get("trinfo") if isinstance(vp, dict) else None
    return None if tr is None or len(tr) == 0 else tr


def trinfo_row(tr, name, D):
    return np.asarray(tr[name], dtype=np.float64).reshape(D)


def trinfo_scale(tr, D):
    """warpvars_vbmc.m:66-69: the scale row counts only where it differs from one"""
    sc = tr.get("scale")
    if sc is None or np.size(sc) == 0:
        return None
    sc = np.asarray(sc, dtype=np.float64).reshape(D)
    return sc if np.any(sc != 1) else None


def trinfo_rot(tr, D):
    R = tr.get("R_mat")
    return None if R is None or np.size(R) == 0 else np.asarray(R, dtype=np.float64).reshape(D, D)


class Desc:
    """A vbmc_vp_desc and the arrays it points at"""

    def __init__(self, vp):
        D, K = int(vp["D"]), int(vp["K"])
        self.D, self.K = D, K
        d = new_args(VpDesc)
        d.D, d.K = D, K
        self.keep = list(mixture(vp, d, prefix=""))
        tr = trinfo_of(vp)
        if tr is not None:
            typ = np.ascontiguousarray(np.asarray(tr["type"]).reshape(D).astype(np.int32))
            rows = [f64(trinfo_row(tr, n, D)) for n in ("lb_orig", "ub_orig", "mu", "delta")]
            sc, R = trinfo_scale(tr, D), trinfo_rot(tr, D)
            sc, R = None if sc is None else f64(sc), None if R is None else f64(R)
            self.keep += [typ, sc, R] + rows
            d.type = typ.ctypes.data_as(i32p)
            d.lb, d.ub, d.tmu, d.tdelta = (ptr(r) for r in rows)
            d.scale, d.R = ptr(sc), ptr(R)
        self.d = d

    def ref(self):
        return C.byref(self.d)

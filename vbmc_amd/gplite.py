"""gplite GP surrogate on the GPU behind the reference's call surface.

``gplite_post(hyp, X, y, covfun, meanfun, noisefun, s2)`` (gplite/gplite_post.m:1),
``gplite_pred(gp, Xstar, ystar, s2star, ssflag)`` (gplite/gplite_pred.m:1) and
``gplite_nlZ(hyp, gp, hprior)`` (gplite/gplite_nlZ.m:1), ``gplite_hypprior(hyp, hprior)``
(gplite/gplite_hypprior.m:1) and ``sq_dist(a, b)`` (utils/sq_dist.m:14) keep the reference's positional arguments.  ``gp`` is a
dict with the reference's field names; its ``post`` list holds the per-hyper-sample
{hyp, alpha, sW, L, sn2_mult, Lchol} exactly like ``gp.post(s)``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _pack
from ._lib import (VBMC_ERR_UNSUPPORTED, DeviceGP, GpTrainArgs, GsArgs, PredPlanInfo, SliceArgs, VbmcUnsupported, f64, host_dump, new_args,
                   ptr)
from .elbo import default_engine
from .ensemble import ensemble_slice_sample


def _nnoise(noisefun):
    return int(noisefun[0] == 1) + int(noisefun[1] == 2) + 2 * int(len(noisefun) > 2 and noisefun[2] == 1)


def _nmean(meanfun, D):
    return {0: 0, 1: 1, 4: 2 * D + 1}.get(int(meanfun), -1)


def sq_dist(a, b=None, *, engine=None):
    """C = sq_dist(a, b): pairwise squared distances between the columns of a (D x n) and b (D x m)."""
    engine = engine or default_engine()
    ctx = engine.ctx
    a = f64(a)
    D, n = a.shape
    if b is None:
        m, bp = n, None
    else:
        b = f64(b)
        if b.shape[0] != D:
            raise ValueError("Error: column lengths must agree.")  # sq_dist.m:35
        m, bp = b.shape[1], ptr(b)
    Cm = np.zeros((n, m), dtype=np.float64, order="F")
    ctx.check(ctx.lib.vbmc_sq_dist(ctx.h, D, n, m, ptr(a), bp, ptr(Cm)))
    return Cm


def gplite_post(hyp, X, y, covfun=1, meanfun=1, noisefun=None, s2=None, *, need_L=True, engine=None):
    """gp = gplite_post(hyp,X,y,covfun,meanfun,noisefun,s2): full posterior for every hyper-sample.

    ``need_L=False`` keeps the N x N x S factors on the device only (``post[s]["L"]`` is None): every accelerated consumer
    (gplite_pred, the ELBO, the acquisition sweep, the rank-one append) reads the device copy, and the 8 N^2 S bytes of
    readback -- 25.6 MB at N = 400, S = 20, most of the call's wall time -- are skipped.

    Only the VBMC configuration is accelerated: covfun 1 (SE-ARD), meanfun in {0, 1, 4}; anything
    else raises VbmcUnsupported so a caller can fall through to the reference implementation.
    """
    engine = engine or default_engine()
    ctx = engine.ctx
    X = f64(X)
    N, D = X.shape
    y = f64(np.asarray(y, dtype=np.float64).reshape(-1))
    hyp = f64(np.asarray(hyp, dtype=np.float64))
    if hyp.ndim == 1:
        hyp = f64(hyp.reshape(-1, 1))
    Nhyp, S = hyp.shape
    if covfun is None:
        covfun = 1
    if np.ndim(covfun) and len(covfun):
        covfun = covfun[0]
    if int(covfun) != 1:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "only the SE-ARD covariance (covfun 1) is accelerated")
    if meanfun is None:
        meanfun = 1  # gplite_post.m:103
    if noisefun is None:
        noisefun = (1, 0, 0) if s2 is None else (1, 1, 0)  # :104-106
    noisefun = tuple(int(v) for v in noisefun) + (0,) * (3 - len(noisefun))
    s2a = None if s2 is None else f64(np.asarray(s2, dtype=np.float64).reshape(-1))
    alpha = np.empty((N, S), order="F")      # all three are overwritten in full by the library
    L = np.empty((N, N, S), order="F") if need_L else None
    sW = np.empty((N, S), order="F")
    mult = np.zeros(S)
    lch = np.zeros(S, dtype=np.uint8)
    nf = (C.c_int32 * 3)(*noisefun)
    h = C.c_void_p()
    ctx.check(ctx.lib.vbmc_gp_post(ctx.h, N, D, S, Nhyp, int(meanfun), nf, ptr(X), ptr(y), ptr(s2a), ptr(hyp), ptr(alpha),
                                   ptr(L), ptr(sW), ptr(mult), lch.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h)))
    gp = {
        "X": X, "y": y, "s2": s2a, "covfun": 1, "meanfun": int(meanfun), "noisefun": noisefun,
        "Ncov": D + 1, "Nnoise": _nnoise(noisefun), "Nmean": _nmean(meanfun, D), "meanfun_extras": None, "intmeanfun": 0,
        # L[:, :, s] is a contiguous (column-major) view of the N x N x S block written by the library: no second copy
        "post": [{"hyp": hyp[:, s].copy(), "alpha": alpha[:, s].copy(), "sW": sW[:, s].copy(), "L": L[:, :, s] if need_L else None,
                  "sn2_mult": float(mult[s]), "Lchol": bool(lch[s])} for s in range(S)],
    }
    dgp = DeviceGP.from_handle(ctx, h, N, D, S)
    engine._remember(gp, dgp, True)
    return gp


def _device_gp_with_noise(engine, gp):
    dgp = engine.device_gp(gp, need_L=True)
    dgp.set_noise(gp["noisefun"], [p["sn2_mult"] for p in gp["post"]])
    return dgp


def gplite_pred(gp, Xstar, ystar=None, s2star=None, ssflag=False, nowarpflag=False, nargout=4, *, engine=None):
    """[ymu,ys2,fmu,fs2,lp] = gplite_pred(gp,Xstar,ystar,s2star,ssflag).  ``nargout=5`` with ``ystar`` adds the log
    predictive density lp (Nstar x S, per hyper-sample also when the other outputs are averaged: gplite_pred.m:124-127)."""
    if nargout > 4:
        Ns = np.asarray(Xstar).shape[0]
        if ystar is not None and np.size(ystar) and np.asarray(ystar).reshape(-1).shape[0] != Ns:
            raise ValueError("gplite_pred:ydimmismatch YSTAR should be empty or a column vector of NSTAR observations.")
        ymu_s, ys2_s = gplite_pred(gp, Xstar, ystar, s2star, True, nowarpflag, 2, engine=engine)
        lp = None
        if ystar is not None and np.size(ystar):
            ymu_s = np.asarray(ymu_s).reshape(Ns, -1)
            ys2_s = np.asarray(ys2_s).reshape(Ns, -1)
            yv = np.asarray(ystar, dtype=np.float64).reshape(-1, 1)
            lp = -0.5 * (yv - ymu_s) ** 2 / ys2_s - 0.5 * np.log(2 * np.pi * ys2_s)   # O(Nstar S) on the host
        return tuple(gplite_pred(gp, Xstar, ystar, s2star, ssflag, nowarpflag, 4, engine=engine)) + (lp,)
    engine = engine or default_engine()
    ctx = engine.ctx
    Xs = f64(Xstar)
    Nstar = Xs.shape[0]
    if s2star is not None and np.size(s2star) and np.asarray(s2star).reshape(-1).shape[0] != Nstar:
        raise ValueError("gplite_pred:s2dimmismatch S2STAR should be empty or a column vector of NSTAR estimated variances.")
    s2s = None if s2star is None or np.size(s2star) == 0 else f64(np.asarray(s2star, dtype=np.float64).reshape(-1))
    if ystar is not None and np.size(ystar) and np.asarray(ystar).reshape(-1).shape[0] != Nstar:
        raise ValueError("gplite_pred:ydimmismatch YSTAR should be empty or a column vector of NSTAR observations.")
    # ystar only matters for output-dependent noise at the test points (gplite_noisefun.m:198-207)
    ys = None if ystar is None or np.size(ystar) == 0 else f64(np.asarray(ystar, dtype=np.float64).reshape(-1))
    dgp = _device_gp_with_noise(engine, gp)
    S = dgp.S
    per = bool(ssflag) or S == 1
    shape = (Nstar, S) if (per and S > 1) else (Nstar,)
    outs = [np.zeros((Nstar, S) if per else (Nstar,), order="F") for _ in range(4)]
    ctx.check(ctx.lib.vbmc_gp_pred(ctx.h, dgp.h, Nstar, ptr(Xs), ptr(ys), ptr(s2s), 1 if per else 0, ptr(outs[0]), ptr(outs[1]),
                                   ptr(outs[2]), ptr(outs[3])))
    outs = [o.reshape(shape, order="F") if per else o for o in outs]
    return tuple(outs[: max(1, nargout)])


def gplite_pred_device(gp, Xs, engine):
    """[ymu,ys2,fmu,fs2] = gplite_pred(gp,Xs,[],[],1,0) per hyper-sample (Nstar x S) on the device."""
    out = gplite_pred(gp, Xs, None, None, True, False, 4, engine=engine)
    S = len(gp["post"])
    return tuple(np.asarray(o).reshape(np.asarray(Xs).shape[0], S) for o in out)


def pred_plan(gp, Nstar, want_ks=False, quad=False, *, engine=None):
    """The launch form one ``gplite_pred`` (``quad``: ``gplite_quad``) call on ``Nstar`` points takes on this device, as a dict of
    the fields of vbmc_pred_plan_info (include/vbmc_hip.h); ``want_ks`` for the form behind the IQR acquisition functions.  Launches
    nothing: the reporting hook vbmc_pred_plan evaluates the functions the launch itself reads."""
    engine = engine or default_engine()
    ctx = engine.ctx
    dgp = _device_gp_with_noise(engine, gp)
    info = new_args(PredPlanInfo)
    ctx.check(ctx.lib.vbmc_pred_plan(ctx.h, dgp.h, int(Nstar), 1 if want_ks else 0, 1 if quad else 0, C.byref(info)))
    return {n: int(getattr(info, n)) for n, _ in PredPlanInfo._fields_[1:]}


def gplite_quad(gp, mu, sigma, ssflag=False, nargout=2, *, engine=None):
    """[F,varF] = gplite_quad(gp,mu,sigma,ssflag)  (gplite/gplite_quad.m:1-119): Bayesian quadrature of the GP against
    N(mu_i, diag sigma^2) for every row of ``mu`` (Nstar x D).  ``sigma`` is a row of D values shared by all points, or an
    Nstar x D matrix whose rows are all equal (collapsed to that row); distinct rows raise VbmcUnsupported.  Averaged over the
    hyper-samples unless ``ssflag`` (:112-119); ``nargout=1`` skips the variance's readback."""
    engine = engine or default_engine()
    ctx = engine.ctx
    D = gp["X"].shape[1]
    if int(np.ravel(gp.get("covfun", 1))[0]) != 1:   # :21-24
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_quad: Bayesian quadrature only supports the squared exponential kernel")
    if int(gp["meanfun"]) not in (0, 1, 4):    # the reference also admits 6 and 8 (:16-19): not accelerated
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_quad: mean function %d is not accelerated (0, 1, 4)" % int(gp["meanfun"]))
    mu = f64(np.asarray(mu, dtype=np.float64).reshape(-1, D))
    Nstar = mu.shape[0]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1, D)
    if sigma.shape[0] not in (1, Nstar):
        raise ValueError("gplite_quad: SIGMA should be a row of D values or an NSTAR x D matrix")
    if sigma.shape[0] > 1:
        if not np.all(sigma == sigma[:1]):
            raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_quad: a sigma row per point is not accelerated (one shared row only)")
        sigma = sigma[:1]
    sigma = f64(sigma)
    dgp = _device_gp_with_noise(engine, gp)
    S = dgp.S
    per = bool(ssflag) or S == 1
    shape = (Nstar, S) if per else (Nstar,)
    F = np.zeros(shape, order="F")
    varF = np.zeros(shape, order="F") if nargout > 1 else None
    ctx.check(ctx.lib.vbmc_gp_quad(ctx.h, dgp.h, Nstar, ptr(mu), ptr(sigma), 1, 1 if per else 0, ptr(F), ptr(varF)))
    return (F, varF) if nargout > 1 else F


def gplite_post_rank1(gp, xstar, ystar, s2star=None, *, need_L=True, engine=None):
    """gp = gplite_post(gp, xstar, ystar, [], [], [], [], 1): rank-1 append of one observation
    (gplite/gplite_post.m:173-251).  Falls back to the full update when ``s2`` is present, as the
    reference does (:76-79).  need_L=False leaves post[s]["L"] = None on the host: the updated factors stay on the
    device, where this package's own consumers (gplite_pred, acqwrapper_vbmc, negelcbo_vbmc, the next append) read them."""
    engine = engine or default_engine()
    ctx = engine.ctx
    xstar = np.asarray(xstar, dtype=np.float64).reshape(1, -1)
    ystar = float(np.asarray(ystar).reshape(-1)[0])
    has_s2 = gp.get("s2") is not None and np.size(gp["s2"]) > 0
    new_s2 = s2star is not None and np.size(s2star) > 0
    if has_s2 != new_s2:
        raise ValueError("gplite_post: the new observation %s an estimated variance s2star but gp.s2 is %s"
                         % ("has" if new_s2 else "lacks", "empty" if not has_s2 else "set"))
    if new_s2:  # heteroskedastic noise: the reference leaves the rank-1 path when the new s2 is non-empty (:76-79,86-90)
        hyp = np.stack([p["hyp"] for p in gp["post"]], axis=1)
        s2new = np.concatenate([np.asarray(gp["s2"], dtype=np.float64).reshape(-1), [float(np.asarray(s2star).reshape(-1)[0])]])
        return gplite_post(hyp, np.vstack([gp["X"], xstar]), np.concatenate([gp["y"], [ystar]]), 1, gp["meanfun"],
                           gp["noisefun"], s2new, engine=engine)
    N, D = np.asarray(gp["X"]).shape
    S = len(gp["post"])
    # [mstar, vstar] of :189 are formed inside the library from the solves of the append itself
    dgp = _device_gp_with_noise(engine, gp)
    Ncov = gp["Ncov"]
    sn2_eff = np.zeros(S)
    for s, post in enumerate(gp["post"]):
        hyp = post["hyp"]
        sn2 = math.exp(2.0 * hyp[Ncov]) if gp["noisefun"][0] == 1 else float(np.finfo(np.float64).eps)
        if len(gp["noisefun"]) > 2 and gp["noisefun"][2] == 1:
            off = Ncov + (1 if gp["noisefun"][0] == 1 else 0) + (1 if gp["noisefun"][1] == 2 else 0)
            sn2 += math.exp(2.0 * hyp[off + 1]) * max(0.0, hyp[off] - ystar) ** 2
        sn2_eff[s] = sn2 * post["sn2_mult"]                                           # :207
    # the append itself runs on the device (k_rank1_assemble) and yields a new surrogate handle; L crosses PCIe only if wanted
    Xn = f64(np.vstack([gp["X"], xstar]))
    alpha = np.empty((N + 1, S), order="F")
    Lh = np.empty((N + 1, N + 1, S), order="F") if need_L else None
    h = C.c_void_p()
    ctx.check(ctx.lib.vbmc_gp_rank1_update(ctx.h, dgp.h, ptr(Xn), C.c_double(ystar), None, None, ptr(f64(sn2_eff)), ptr(alpha),
                                           ptr(Lh) if need_L else None, C.byref(h)))
    out = {k: v for k, v in gp.items() if k != "post"}
    out["X"] = Xn
    out["y"] = np.concatenate([gp["y"], [ystar]])
    out["post"] = [{"hyp": p["hyp"].copy(), "alpha": alpha[:, s].copy(),
                    "sW": np.concatenate([p["sW"], [1.0 / math.sqrt(sn2_eff[s])]]),   # :239
                    "L": Lh[:, :, s] if need_L else None, "sn2_mult": p["sn2_mult"], "Lchol": p["Lchol"]}
                   for s, p in enumerate(gp["post"])]
    ndgp = DeviceGP.from_handle(ctx, h, N + 1, D, S)
    ndgp.set_noise(gp["noisefun"], [p["sn2_mult"] for p in gp["post"]])
    engine._remember(out, ndgp, True)
    return out


def gplite_hypprior(hyp, hprior, nargout=2):
    """[lp,dlp] = gplite_hypprior(hyp,hprior)  (gplite/gplite_hypprior.m:17-65): independent flat / Gaussian /
    Student-t log-priors per hyper-parameter.  O(Nhyp) host arithmetic, no device work."""
    lgamma, pi = math.lgamma, math.pi
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.ndim == 2 and hyp.shape[1] > 1:
        raise ValueError("gplite_hypprior:nosampling Hyperparameter log priors are available only for one-sample hyperparameter inputs.")
    hyp = hyp.reshape(-1)
    n = hyp.size
    mu = np.asarray(hprior["mu"], dtype=np.float64).reshape(-1)
    sigma = np.abs(np.asarray(hprior["sigma"], dtype=np.float64).reshape(-1))
    df = hprior.get("df")
    df = np.full(n, 7.0) if df is None or np.size(df) == 0 else np.asarray(df, dtype=np.float64).reshape(-1)
    flat = ~np.isfinite(mu) | ~np.isfinite(sigma)
    gauss = ~flat & ((df == 0) | ~np.isfinite(df)) & np.isfinite(sigma)
    stud = ~flat & (df > 0) & np.isfinite(df)
    dev = np.zeros(n)
    sel = gauss | stud
    dev[sel] = (hyp[sel] - mu[sel]) / sigma[sel]
    z2 = dev * dev
    lp = -0.5 * float(np.sum(np.log(2 * pi * sigma[gauss] ** 2) + z2[gauss]))
    dlp = np.zeros(n)
    dlp[gauss] = -dev[gauss] / sigma[gauss]
    if np.any(stud):
        nu = df[stud]
        const = np.array([lgamma(0.5 * (v + 1)) - lgamma(0.5 * v) for v in nu]) - 0.5 * np.log(pi * nu) - np.log(sigma[stud])
        lp += float(np.sum(const - 0.5 * (nu + 1) * np.log1p(z2[stud] / nu)))
        dlp[stud] = -(nu + 1) / nu / (1 + z2[stud] / nu) * dev[stud] / sigma[stud]
    return (lp, dlp) if nargout > 1 else lp


def gplite_nlZ(hyp, gp, hprior=None, nargout=2, *, engine=None):
    """[nlZ,dnlZ] = gplite_nlZ(hyp,gp,hprior)  (gplite/gplite_nlZ.m:1-72).

    ``hyp`` Nhyp (or Nhyp x 1) follows the reference: scalar nlZ and an Nhyp gradient.  Beyond the reference,
    ``hyp`` Nhyp x B with B > 1 evaluates all B vectors (the walkers / restarts of gplite_train.m:181,251,292)
    in ONE batched device pass and returns nlZ (B) and dnlZ (Nhyp x B); the reference raises
    gplite_nlZ:NoSampling for that form when a gradient is requested (:41-44).
    """
    engine = engine or default_engine()
    ctx = engine.ctx
    X = f64(gp["X"])
    N, D = X.shape
    y = f64(np.asarray(gp["y"], dtype=np.float64).reshape(-1))
    s2 = gp.get("s2")
    s2 = None if s2 is None or np.size(s2) == 0 else f64(np.asarray(s2, dtype=np.float64).reshape(-1))
    H = np.asarray(hyp, dtype=np.float64)
    single = H.ndim == 1 or H.shape[1] == 1
    H = f64(H.reshape(H.shape[0], -1))
    Nhyp, B = H.shape
    noisefun = tuple(gp["noisefun"])
    if Nhyp != gp["Ncov"] + gp["Nnoise"] + gp["Nmean"]:
        raise ValueError("gplite_nlZ:dimmismatch Number of hyperparameters mismatched with dimension of training inputs.")
    if gp.get("intmeanfun", 0) or gp.get("outwarpfun") is not None or int(np.atleast_1d(gp.get("covfun", 1))[0]) != 1:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_nlZ: integrated mean / output warping / non-SE covariance are not accelerated")
    nf = (C.c_int32 * 3)(*[int(v) for v in (list(noisefun) + [0, 0, 0])[:3]])
    grad = nargout > 1
    nlZ = np.zeros(B)
    dnlZ = np.zeros((Nhyp, B), order="F") if grad else None
    ctx.check(ctx.lib.vbmc_gp_nlz(ctx.h, N, D, B, Nhyp, int(gp["meanfun"]), nf, ptr(X), ptr(y), ptr(s2), ptr(H), int(grad),
                                  ptr(nlZ), ptr(dnlZ)))
    if hprior is not None:
        for b in range(B):
            P, dP = gplite_hypprior(H[:, b], hprior)
            nlZ[b] -= P
            if grad:
                dnlZ[:, b] -= dP
    if single:
        return (float(nlZ[0]), dnlZ[:, 0].copy()) if grad else float(nlZ[0])
    return (nlZ, dnlZ) if grad else nlZ


def slice_rng_dump(seed, sweeps, Nhyp, Kmax):
    """(perms, U): the 0-based permutations (sweeps x Nhyp, int32) and the indexed uniform block U[sweep, idd, slot]
    (sweeps x Nhyp x (2 + Kmax)) that ``seed`` stands for in the device-RNG mode of slicesamplebnd_gp (vbmc_slice_rng_dump: a
    host function).  Feeding them back as ``perms=`` / ``uniforms=`` replays the chain bit for bit."""
    perms = np.zeros((int(sweeps), int(Nhyp)), dtype=np.int32)
    U = np.zeros((int(sweeps), int(Nhyp), 2 + int(Kmax)))
    host_dump("vbmc_slice_rng_dump", seed, sweeps, Nhyp, Kmax, perms, U)
    return perms, U


class SliceOutput(dict):
    """The reference's fourth output (output.widths, output.funccount) plus the device chain's own counters."""
    __getattr__ = dict.__getitem__


def slicesamplebnd_gp(gp, hprior, x0, N, widths=None, LB=None, UB=None, options=None, *, seed=0, uniforms=None, perms=None, W=None,
                      engine=None):
    """[samples,fvals,exitflag,output] = slicesamplebnd(@(hyp) gp_objfun(hyp(:),gp,hprior,0,1), x0, N, widths, LB, UB, options)
    (utils/slicesamplebnd.m:1, the call of gplite/gplite_train.m:318-330) with the whole chain on the device.

    ``options``: Thin (1), Burnin (round(N/3)), Adaptive (True) as in the reference (:143-147); StepOut must stay false, Display and
    Diagnostics are not offered (exitflag is 0, as with Diagnostics = false, :395).  Random numbers: the library's generator keyed by
    ``seed``, or -- parity mode -- the caller's ``perms`` (sweeps x Nhyp, 0-based) and ``uniforms`` (sweeps x Nhyp x (2 + Kmax), see
    include/vbmc_hip.h).  ``W``: speculation width (None: the library's default); every W returns the same bits.
    ``output``: widths, funccount (evaluations of the sequential algorithm), performed (evaluations launched), maxshrink,
    rounds_done / rounds_enqueued (rounds of the device chain that did work / that the host enqueued)."""
    engine = engine or default_engine()
    ctx = engine.ctx
    options = dict(options or {})
    if options.get("StepOut"):
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "slicesamplebnd_gp: the step-out procedure is not accelerated")
    a = new_args(SliceArgs)
    keep = [_pack.training_block(a, gp, "slicesamplebnd_gp")]
    x0 = f64(np.asarray(x0, dtype=np.float64).reshape(-1))
    Nhyp = a.Nhyp = x0.size
    lb, ub = _pack.box(LB, UB, Nhyp, open_ended=True)
    base = None
    if widths is None or np.size(widths) == 0:
        wd = (ub - lb) / 2                                                       # :173-174
        wd[np.isinf(wd)] = 10.0
    else:
        wd = _pack.row(widths, Nhyp)
        base = f64(wd.copy())                                                    # :166
    wd = f64(wd)
    N = int(N)
    thin = int(np.floor(options.get("Thin", 1)))
    burn = int(np.floor(options.get("Burnin", round(N / 3))))
    keep.append(_pack.hyper_prior(a, hprior, Nhyp, "slicesamplebnd_gp"))
    a.LB, a.UB, a.hyp_start, a.widths, a.basewidths = ptr(lb), ptr(ub), ptr(x0), ptr(wd), ptr(base)
    a.Ns, a.Thin, a.Burnin, a.Adaptive = N, thin, burn, int(bool(options.get("Adaptive", True)))
    a.W = 0 if W is None else int(W)
    if uniforms is not None or perms is not None:
        if uniforms is None or perms is None:
            raise ValueError("slicesamplebnd_gp: parity mode needs both perms and uniforms")
        sweeps = burn + N + (N - 1) * (thin - 1)
        U = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64))
        P = np.ascontiguousarray(np.asarray(perms, dtype=np.int32))
        if U.ndim != 3 or U.shape[0] < sweeps or U.shape[1] != Nhyp or U.shape[2] < 3 or P.shape[0] < sweeps or P.shape[1:] != (Nhyp,):
            raise ValueError("slicesamplebnd_gp: uniforms must be sweeps x Nhyp x (2 + Kmax) and perms sweeps x Nhyp for %d sweeps" % sweeps)
        keep += [U, P]
        a.rng_mode, a.Kmax = 1, U.shape[2] - 2
        a.perms, a.uniforms = P.ctypes.data_as(_pack.i32p), ptr(U)
    else:
        a.rng_mode, a.seed = 0, int(seed)
    samples = np.zeros((N, Nhyp), order="F")
    logp = np.zeros(N)
    wout = np.zeros(Nhyp)
    ms = C.c_int32(0)
    a.samples, a.logp, a.widths_out, a.max_shrink = ptr(samples), ptr(logp), ptr(wout), C.pointer(ms)
    counts = _pack.counters(a)
    ctx.check(ctx.lib.vbmc_gp_slice_sample(ctx.h, C.byref(a)))
    c = counts()                                         # (the second slot of rounds[] counts the rounds enqueued here)
    out = SliceOutput(widths=wout, funccount=c["funccount"], performed=c["performed"], maxshrink=int(ms.value), logpriors=None,
                      rounds_done=c["rounds"], rounds_enqueued=c["behind"])
    return samples, logp, 0, out


def gplite_train_sample(gp, hyp_start, Ns, hprior=None, LB=None, UB=None, widths=None, *, Thin=1, Burnin=None, seed=0, uniforms=None,
                        perms=None, W=None, need_L=True, engine=None):
    """The sampling half of gplite_train (gplite/gplite_train.m:303-340, sampler 'slicesample'), the thinning that follows it
    (:459-461) and the closing gplite_post of the thinned samples (:474): ``Ns * Thin`` sweeps are recorded after ``Burnin``
    (default: Thin * Ns, :51), every Thin-th is kept, and the returned ``gp`` holds the Ns hyper-samples with its posterior on the
    device (``need_L`` as in gplite_post).  The optimisation half (:200-306) is not part of this package: ``hyp_start`` is the caller's.
    Returns (gp, hyp, output): hyp Nhyp x Ns, output = {hyp_prethin, logp, logp_prethin, widths, funccount, performed, maxshrink}."""
    hyp_start = np.asarray(hyp_start, dtype=np.float64).reshape(-1)
    Nhyp = hyp_start.size
    Ns, Thin = int(Ns), int(Thin)
    if Ns < 1 or Thin < 1:
        raise ValueError("gplite_train_sample: Ns and Thin must be positive")
    Burnin = Thin * Ns if Burnin is None else int(Burnin)
    lb, ub = _pack.box(LB, UB, Nhyp, open_ended=True)
    # the starting point inside the bounds, fixed coordinates at their value (:304-306)
    with np.errstate(invalid="ignore"):
        elb = np.where(np.isfinite(lb), np.spacing(np.abs(lb)), 0.0)
        eub = np.where(np.isfinite(ub), np.spacing(np.abs(ub)), 0.0)
    x0 = np.minimum(np.maximum(hyp_start, lb + elb), ub - eub)
    fixed = lb == ub
    x0[fixed] = lb[fixed]
    samples, fvals, _, out = slicesamplebnd_gp(gp, hprior, x0, Ns * Thin, widths, lb, ub, {"Thin": 1, "Burnin": Burnin}, seed=seed,
                                               uniforms=uniforms, perms=perms, W=W, engine=engine)
    hyp_prethin = np.ascontiguousarray(samples.T)
    hyp = hyp_prethin[:, Thin - 1::Thin].copy()
    new = gplite_post(hyp, gp["X"], gp["y"], 1, gp["meanfun"], gp["noisefun"], gp.get("s2"), need_L=need_L, engine=engine)
    output = {"hyp_prethin": hyp_prethin, "logp": fvals[Thin - 1::Thin].copy(), "logp_prethin": fvals, "widths": out["widths"],
              "funccount": out["funccount"], "performed": out["performed"], "maxshrink": out["maxshrink"]}
    return new, hyp, output


def _uuinv(p, B, w):
    """Inverse cdf of w U(B2, B3) + (1 - w)/2 (U(B1, B2) + U(B3, B4))   (utils/fminfill.m:132-171)"""
    p = np.asarray(p, dtype=np.float64)
    x = np.zeros_like(p)
    L = B[3] - B[0] + B[1] - B[2]
    if w == 1:
        return p * (B[2] - B[1]) + B[1]
    if L == 0:   # a delta at either end and the uniform between
        i1 = p <= (1 - w) / 2
        x[i1] = B[0]
        if w != 0:
            i2 = (p <= (1 - w) / 2 + w) & ~i1
            x[i2] = (p[i2] - (1 - w) / 2) * (B[2] - B[1]) / w + B[1]
        x[p > (1 - w) / 2 + w] = B[3]
        return x
    t1 = (1 - w) * (B[1] - B[0]) / L
    i1 = p <= t1
    x[i1] = B[0] + p[i1] * L / (1 - w)
    i2 = (p <= t1 + w) & ~i1
    if w != 0:
        x[i2] = (p[i2] - t1) * (B[2] - B[1]) / w + B[1]
    i3 = p > t1 + w
    x[i3] = (p[i3] - w - t1) * L / (1 - w) + B[2]
    x[(p < 0) | (p > 1)] = np.nan
    return x


def fminfill_design(hyp0, LB, UB, PLB, PUB, hprior, Ninit, S=None, *, seed=0):
    """The points fminfill evaluates (utils/fminfill.m:42-101): the rows of ``hyp0`` (N0 x Nhyp) moved inside the bounds, then
    Ninit - N0 points mapped from the unit-cube block ``S`` -- the mixture of uniforms over the hard and the plausible box for a
    coordinate without a prior, the truncated Student-t quantile (df capped at 3, df = 0: normal) for one with a prior.  ``S``
    defaults to uniform random numbers (VBMC's own design, 'rand', vbmc.m:238); a caller who wants a Sobol design passes its block.
    Returns Ninit x Nhyp (max(Ninit, N0) rows when hyp0 holds more than Ninit)."""
    x0 = np.atleast_2d(np.asarray(hyp0, dtype=np.float64))
    nvars = x0.shape[1]
    LB, UB = _pack.box(LB, UB, nvars, open_ended=True)
    PLB, PUB = _pack.row(PLB, nvars, LB), _pack.row(PUB, nvars, UB)
    x0 = np.maximum(np.minimum(x0, UB), LB)                                      # :44
    N0, Ninit = x0.shape[0], int(Ninit)
    if Ninit <= N0:
        return x0
    hprior = hprior or {}
    pad = lambda v: np.concatenate([np.asarray([] if v is None else v, dtype=np.float64).reshape(-1), np.full(nvars, np.nan)])[:nvars]
    mu, sigma, dfs = pad(hprior.get("mu")), pad(hprior.get("sigma")), pad(hprior.get("df"))
    if S is None:
        S = np.random.default_rng(seed).random((Ninit - N0, nvars))
    S = np.asarray(S, dtype=np.float64)
    if S.shape != (Ninit - N0, nvars):
        raise ValueError("fminfill_design: S must be (Ninit - N0) x Nhyp = %d x %d" % (Ninit - N0, nvars))
    Xs = np.zeros((Ninit - N0, nvars))
    for i in range(nvars):
        if not np.isfinite(mu[i]) or not np.isfinite(sigma[i]):
            if np.isfinite(LB[i]) and np.isfinite(UB[i]):
                Xs[:, i] = _uuinv(S[:, i], [LB[i], PLB[i], PUB[i], UB[i]], 0.5 ** (1.0 / nvars))   # :77-78
            else:
                Xs[:, i] = S[:, i] * (PUB[i] - PLB[i]) + PLB[i]                  # :81
        else:
            from scipy import special as sp                                      # lazy: only a design with a prior needs it

            df = dfs[i] if np.isfinite(dfs[i]) else 3.0                          # :85-88
            df = min(df, 3.0)
            if df == 0:
                cdf, inv = sp.ndtr, sp.ndtri
            else:
                cdf, inv = (lambda z, v=df: sp.stdtr(v, z)), (lambda q, v=df: sp.stdtrit(v, q))
            lo, hi = cdf((LB[i] - mu[i]) / sigma[i]), cdf((UB[i] - mu[i]) / sigma[i])
            Xs[:, i] = inv(lo + (hi - lo) * S[:, i]) * sigma[i] + mu[i]          # :90-93
    return np.vstack([x0, Xs])


def gplite_train_optimize(gp, hyp0, LB, UB, PLB=None, PUB=None, hprior=None, options=None, *, engine=None):
    """The optimisation half of gplite_train (gplite/gplite_train.m:200-306) in ONE device call (vbmc_gp_train_optimize): fill
    stage over ``fminfill_design``, the starts, the library's own projected-BFGS optimiser from all Nopts starts in lock-step, the
    closing.  ``hyp0``: Nhyp or Nhyp x N0 as in the reference.  ``options``: Ninit (1024), Nopts (3), TolFun (1e-5), MaxIter (1000),
    MaxFunEvals (3000), W (library default), S / seed (the unit-cube block of the design or the seed of its uniform default),
    Design (the finished Ninit x Nhyp design, instead of S), History (iterations per start to record, 0).
    Returns a dict: hyp (Nhyp x Nopts), nll, best, hyp_start, widths_default, fill_fvals, fill_order, design, iterations,
    funccount, exitflag, performed and, with History, hist_x (Nopts x History x Nhyp), hist_f, hist_k."""
    engine = engine or default_engine()
    ctx = engine.ctx
    options = dict(options or {})
    a = new_args(GpTrainArgs)
    keep = [_pack.training_block(a, gp, "gplite_train_optimize")]
    H0 = np.asarray(hyp0, dtype=np.float64)
    H0 = H0.reshape(H0.shape[0], -1)
    Nhyp, N0 = H0.shape
    lb, ub = _pack.box(LB, UB, Nhyp, open_ended=True)
    Ninit, Nopts = int(options.get("Ninit", 1024)), int(options.get("Nopts", 3))
    if options.get("Design") is not None:
        design = np.atleast_2d(np.asarray(options["Design"], dtype=np.float64))
        Ninit = design.shape[0]
    elif Ninit > 0:
        design = fminfill_design(H0.T, lb, ub, PLB, PUB, hprior, Ninit, options.get("S"), seed=int(options.get("seed", 0)))
    else:
        design = H0.T.copy()
    design = f64(design)
    rows = design.shape[0]
    if design.ndim != 2 or design.shape[1] != Nhyp or (Ninit > 0 and rows != Ninit):
        raise ValueError("gplite_train_optimize: the design must be Ninit x Nhyp")
    a.Nhyp = Nhyp
    keep.append(_pack.hyper_prior(a, hprior, Nhyp, "gplite_train_optimize", needs_mu=True))
    a.LB, a.UB, a.design = ptr(lb), ptr(ub), ptr(design)
    a.Ninit, a.N0, a.Nopts, a.Ncov = (rows if Ninit > 0 else 0), rows, Nopts, a.D + 1
    a.TolFun = float(options.get("TolFun", 1e-5))
    a.MaxIter, a.MaxFunEvals = int(options.get("MaxIter", 1000)), int(options.get("MaxFunEvals", 3000))
    W = options.get("W")
    a.W = 0 if W is None else int(W)
    cap = int(options.get("History", 0))
    n_o = max(Nopts, 1)
    fs, fo, wd = np.zeros(rows), np.zeros(rows, dtype=np.int32), np.full(Nhyp, np.nan)
    hyp, nll, hs = np.zeros((Nhyp, n_o), order="F"), np.zeros(n_o), np.zeros(Nhyp)
    its, fcs, efs = np.zeros(n_o, dtype=np.int32), np.zeros(n_o, dtype=np.int64), np.zeros(n_o, dtype=np.int32)
    best, perf = C.c_int32(0), C.c_int64(0)
    i32p = _pack.i32p
    a.fill_fvals, a.fill_order, a.widths_default = ptr(fs), fo.ctypes.data_as(i32p), ptr(wd)
    a.hyp, a.nll, a.best, a.hyp_start = ptr(hyp), ptr(nll), C.pointer(best), ptr(hs)
    a.iterations, a.funccount, a.exitflag = its.ctypes.data_as(i32p), fcs.ctypes.data_as(_pack.i64p), efs.ctypes.data_as(i32p)
    a.performed = C.pointer(perf)
    if cap > 0:
        hx, hf, hk = np.zeros((n_o, cap, Nhyp)), np.zeros((n_o, cap)), np.zeros((n_o, cap), dtype=np.int32)
        a.hist_cap, a.hist_x, a.hist_f, a.hist_k = cap, ptr(hx), ptr(hf), hk.ctypes.data_as(i32p)
    ctx.check(ctx.lib.vbmc_gp_train_optimize(ctx.h, C.byref(a)))
    if Ninit <= 0:   # :255, the zero widths repaired as in :258-267
        wd = _pack.row(PUB, Nhyp, ub) - _pack.row(PLB, Nhyp, lb)
        z = wd == 0
        if np.any(z) and rows > 1:
            wd[z] = np.std(design[fo], axis=0, ddof=1)[z]
        z = wd == 0
        wd[z] = np.minimum(1.0, ub[z] - lb[z])
    out = {"hyp": hyp, "nll": nll, "best": int(best.value), "hyp_start": hs, "widths_default": wd, "fill_fvals": fs, "fill_order": fo,
           "design": design, "iterations": its, "funccount": fcs, "exitflag": efs, "performed": int(perf.value)}
    if cap > 0:
        out.update(hist_x=hx, hist_f=hf, hist_k=hk)
    return out


def gplite_train(hyp0, Ns, X, y, covfun=1, meanfun=None, noisefun=None, s2=None, hprior=None, options=None, *, LB=None, UB=None,
                 PLB=None, PUB=None, need_L=True, engine=None):
    """[gp,hyp,output] = gplite_train(hyp0,Ns,X,y,covfun,meanfun,noisefun,s2,hprior,options)   (gplite/gplite_train.m:1-489)
    on the device: the optimisation half (gplite_train_optimize), then -- Ns > 0 -- the slice-sampling half from its hyp_start
    (gplite_train_sample, widths as in :323-327), or -- Ns = 0 -- the best optimised vector (:463-468), and the closing
    gplite_post (:474).  Out of scope and refused: options.LogP (the ESS short-cut of :179-198), a Sampler other than
    'slicesample', and the covariance / mean / noise-function bound defaults of :95-158 -- the caller passes LB, UB (hprior.LB /
    hprior.UB are read too) and PLB, PUB.  options beyond the reference's: W, seed, S, MaxIter, MaxFunEvals."""
    options = dict(options or {})
    hprior = dict(hprior or {})
    if options.get("LogP") is not None and np.size(options["LogP"]) > 0:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_train: options.LogP (the ESS short-cut of gplite_train.m:179-198) is not accelerated")
    if str(options.get("Sampler", "slicesample")).lower() != "slicesample":
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_train: only the 'slicesample' sampler is accelerated")
    if isinstance(hyp0, dict) or options.get("OutwarpFun") is not None or int(np.atleast_1d(covfun)[0]) != 1:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_train: variational hyp0 / output warping / non-SE covariance are not accelerated")
    LB = hprior.get("LB") if LB is None else LB
    UB = hprior.get("UB") if UB is None else UB
    if LB is None or UB is None or np.size(LB) == 0 or np.size(UB) == 0 or np.any(np.isnan(np.asarray(LB, dtype=np.float64))) \
            or np.any(np.isnan(np.asarray(UB, dtype=np.float64))):
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_train: the bound defaults of gplite_train.m:95-158 are not built: pass LB and UB")
    X = np.asarray(X, dtype=np.float64)
    s2 = None if s2 is None or np.size(s2) == 0 else s2
    meanfun = 1 if meanfun is None else meanfun                                  # :22
    if noisefun is None or np.size(noisefun) == 0:
        noisefun = [1, 0, 0] if s2 is None else [1, 1, 0]                        # :25-27
    H0 = np.asarray(hyp0, dtype=np.float64)
    H0 = H0.reshape(H0.shape[0], -1)
    Nhyp = H0.shape[0]
    Ns = int(Ns)
    nfl = [int(v) for v in (list(noisefun) + [0, 0, 0])[:3]]
    D = X.shape[1]
    Nnoise = (nfl[0] == 1) + (nfl[1] == 2) + 2 * (nfl[2] == 1)
    gp = {"X": X, "y": np.asarray(y, dtype=np.float64).reshape(-1), "s2": s2, "covfun": 1, "meanfun": int(meanfun), "noisefun": nfl,
          "Ncov": D + 1, "Nnoise": Nnoise, "Nmean": Nhyp - D - 1 - Nnoise}
    prior = None
    if hprior.get("mu") is not None and np.size(hprior["mu"]) > 0:
        pad = lambda v: np.concatenate([np.asarray([] if v is None else v, dtype=np.float64).reshape(-1), np.full(Nhyp, np.nan)])[:Nhyp]
        df = pad(hprior.get("df"))
        df[np.isnan(df)] = float(options.get("DfBase", 7))                       # :113-117
        prior = {"mu": pad(hprior.get("mu")), "sigma": pad(hprior.get("sigma")), "df": df}
    LBv, UBv = _pack.box(LB, UB, Nhyp)
    UBv = np.maximum(LBv, UBv)                                                   # :142
    Thin = int(options.get("Thin", 5))
    tol = float(options.get("TolOptMCMC", 1e-3)) if Ns > 0 else float(options.get("TolOpt", 1e-5))     # :163-167
    oo = {"Ninit": int(options.get("Ninit", 2 ** 10)), "Nopts": int(options.get("Nopts", 3)), "TolFun": tol}
    for k in ("W", "seed", "S", "MaxIter", "MaxFunEvals", "Design"):
        if options.get(k) is not None:
            oo[k] = options[k]
    opt = gplite_train_optimize(gp, H0, LBv, UBv, PLB, PUB, prior, oo, engine=engine)
    output = {"LB": LBv, "UB": UBv, "PLB": PLB, "PUB": PUB, "optimize": opt}
    if Ns > 0:
        widths = opt["widths_default"]
        if options.get("Widths") is not None and np.size(options["Widths"]) > 0:
            widths = np.minimum(np.asarray(options["Widths"], dtype=np.float64).reshape(-1), widths)   # :326
        Burnin = options.get("Burnin")
        new, hyp, so = gplite_train_sample(gp, opt["hyp_start"], Ns, prior, LBv, UBv, widths, Thin=Thin, Burnin=Burnin,
                                           seed=int(options.get("seed", 0)), W=options.get("W"), need_L=need_L, engine=engine)
        output.update(hyp_prethin=so["hyp_prethin"], logp=so["logp"], logp_prethin=so["logp_prethin"])
        return new, hyp, output
    idx = opt["best"]
    hyp = opt["hyp"][:, idx:idx + 1].copy()                                      # :464-467
    new = gplite_post(hyp, X, gp["y"], 1, gp["meanfun"], nfl, s2, need_L=need_L, engine=engine)
    output.update(hyp_prethin=hyp, logp=-opt["nll"][idx], logp_prethin=-opt["nll"])
    return new, hyp, output


def gp_surrogate_sample_rng_dump(seed, E, H, M):
    """U (64 x H x E x M) that ``gplite_sample_device(..., seed=seed)`` consumes (vbmc_gp_surrogate_sample_rng_dump: a pure host function)."""
    U = np.zeros((64, int(H), int(E), int(M)), order="F")
    host_dump("vbmc_gp_surrogate_sample_rng_dump", seed, E, H, M, U)
    return U


def gplite_sample_device(gp, Ns, LB, UB, *, vp=None, x0=None, E=1, W=0, thin=1, burnin=None, beta=0.0, VarThresh=np.inf, noise=None,
                         origflag=False, spec=0, chunk=0, max_steps=0, max_shrink=0, seed=0, uniforms=None, outputs=("X", "Xt", "logp"),
                         engine=None):
    """The thin ctypes call of ``vbmc_gp_surrogate_sample`` (include/vbmc_hip.h): Ns samples of the GP surrogate's log_gpfun target
    (gplite_sample.m:109-117, the prediction averaged over all hyper-samples) by E ensembles of W walkers, the whole chain on the device.

    ``x0``: E x W x D starting walkers (as ``ensemble_slice_sample`` takes them), or None for draws of ``vp``.  ``noise``: a dict with
    X_rescaled, gplengthscale, sn2new and, optionally, Nnn -- the noise estimate of gpsample_vbmc.m:30-38, which then sets VarThresh.
    ``uniforms`` (64 x H x E x Mmax): parity mode; the library's own generator keyed by ``seed`` otherwise.
    Returns a dict: X (Ns x D), Xt (Nm x D x E), logp (E x Nm), x0 (E x W x D, the clipped start), VarThresh, sn2_avg, sn2_nn (with
    ``noise``), funccount, performed, rounds, behind."""
    engine = engine or default_engine()
    ctx = engine.ctx
    dgp = _device_gp_with_noise(engine, gp)
    D, S = int(np.asarray(gp["X"]).shape[1]), len(gp["post"])
    Ns, E = int(Ns), int(E)
    Wn = int(W) if W else 2 * (D + 1)
    keep = list(_pack.box(LB, UB, D))
    a = new_args(GsArgs)
    a.D, a.S, a.E, a.origflag = D, S, E, int(bool(origflag))
    _pack.sampler_opts(a, W, Ns, thin, burnin, spec, max_steps, max_shrink, chunk, seed)
    a.beta, a.VarThresh = float(beta), float(VarThresh)
    a.LB, a.UB = ptr(keep[0]), ptr(keep[1])
    if x0 is not None:
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim == 2:
            x0 = x0[None]
        if x0.ndim != 3 or x0.shape[0] != E or x0.shape[2] != D:
            raise ValueError("gplite_sample_device: x0 must be E x W x D = %d x W x %d" % (E, D))
        Wn = x0.shape[1]
        a.W = Wn
        keep.append(f64(np.transpose(x0, (1, 2, 0))))       # W x D x E
        a.x0 = ptr(keep[-1])
    if uniforms is not None:
        keep.append(_pack.sampler_uniforms(a, uniforms, Wn // 2, E, "gplite_sample_device", axis="E"))
        a.rng_mode = 1
    Nnn = 0
    if noise is not None:
        keep += _pack.nn_noise(a, noise["gplengthscale"], noise["X_rescaled"], noise["sn2new"], np.asarray(gp["X"]).shape[0], D)
        a.Nnn = int(noise.get("Nnn", 0) or 0)
        Nnn = a.Nnn if a.Nnn > 0 else 20000
    desc = None if vp is None else _pack.Desc(vp)
    Nm = max(-(-max(Ns, 1) // max(E, 1)), 1)
    n, Wp, Ep = max(Ns, 1), max(Wn, 1), max(E, 1)
    out = {}
    if "X" in outputs:
        out["X"] = np.zeros((n, D), order="F")
        a.X = ptr(out["X"])
    if "Xt" in outputs:
        out["Xt"] = np.zeros((Nm, D, Ep), order="F")
        a.Xt = ptr(out["Xt"])
    if "logp" in outputs:
        out["logp"] = np.zeros((Ep, Nm), order="F")
        a.logp = ptr(out["logp"])
    x0o = np.zeros((Wp, D, Ep), order="F")
    a.x0_out = ptr(x0o)
    vt, sa = np.zeros(1), np.zeros(1)
    a.varthresh_out, a.sn2_avg_out = ptr(vt), ptr(sa)
    if noise is not None:
        out["sn2_nn"] = np.zeros(Nnn)
        a.sn2_nn = ptr(out["sn2_nn"])
    counts = _pack.counters(a)
    ctx.check(ctx.lib.vbmc_gp_surrogate_sample(ctx.h, dgp.h, desc.ref() if desc is not None else None, C.byref(a)))
    out.update(counts(), x0=np.ascontiguousarray(np.transpose(x0o, (2, 0, 1))), VarThresh=float(vt[0]), sn2_avg=float(sa[0]))
    return out


def _log_gpfun_host(gp, beta, VarThresh, engine):
    """log_gpfun (gplite_sample.m:109-117) over device gplite_pred calls: the target of the host-driven fall-back"""
    plain = (VarThresh == 0 or not np.isfinite(VarThresh)) and beta == 0

    def logp(P, e):
        y, s2 = (np.asarray(v, dtype=np.float64).reshape(-1).copy() for v in gplite_pred(gp, P, None, None, False, False, 2, engine=engine))
        if not plain:
            over = s2 >= VarThresh
            y[over] = y[over] - (s2[over] - VarThresh)
            y = y - beta * np.sqrt(s2)
        return np.where(np.isfinite(y), y, -np.inf)

    return logp


def gplite_sample(gp, Ns, x0=None, method="parallel", logprior=None, beta=0, VarThresh=np.inf, proppdf=None, proprnd=None, bounds=None, *,
                  E=1, seed=0, uniforms=None, thin=1, burnin=None, spec=0, chunk=0, nargout=1, engine=None):
    """Xs = gplite_sample(gp,Ns,x0,method,logprior,beta,VarThresh,proppdf,proprnd,bounds), method 'parallel', on the device: the
    default box (gplite_sample.m:16-20) and the high-posterior-density start of ``x0 = []`` (:88-101, its randperm from a NumPy
    generator keyed by ``seed``) on the host, the chain in one call of ``gplite_sample_device``.  ``x0``: W x D, or E x W x D.
    'slicesample', a ``logprior`` and proposal functions raise VbmcUnsupported.  A GP beyond the range in which the prediction keeps
    inv(L') resident is sampled by the host-driven ``ensemble_slice_sample`` over device ``gplite_pred`` calls.
    nargout=2 adds the dict of ``gplite_sample_device`` (None on the host-driven path)."""
    if method is None or method == "":
        method = "slicesample"                                                   # :5
    if str(method).lower() != "parallel":
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_sample: method %r is not accelerated ('parallel' is)" % (method,))
    if logprior is not None or proppdf is not None or proprnd is not None:
        raise VbmcUnsupported(VBMC_ERR_UNSUPPORTED, "gplite_sample: a logprior and Metropolis proposals are not accelerated")
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    Ns, E = int(Ns), int(E)
    if bounds is None or np.size(bounds) == 0:                                   # :16-20
        diam = np.max(X, axis=0) - np.min(X, axis=0)
        LB, UB = np.min(X, axis=0) - 10 * diam, np.max(X, axis=0) + 10 * diam
    else:
        bounds = np.asarray(bounds, dtype=np.float64).reshape(2, D)
        LB, UB = bounds[0], bounds[1]
    W = 2 * (D + 1)                                                              # :87
    if x0 is None or np.size(x0) == 0:                                           # :88-101
        y = np.asarray(gp["y"], dtype=np.float64).reshape(-1)
        N_hpd = min(N, max(W, int(np.floor(0.25 * N + 0.5))))
        X_hpd = X[np.argsort(-y, kind="stable")[:N_hpd]]
        Wn = min(W, N_hpd) - (min(W, N_hpd) % 2)
        rng = np.random.default_rng(int(seed))
        x0 = np.stack([X_hpd[rng.permutation(N_hpd)[:Wn]] for _ in range(E)])
    else:
        x0 = np.asarray(x0, dtype=np.float64)
        x0 = x0[None] if x0.ndim == 2 else x0
    x0 = np.minimum(np.maximum(x0, LB), UB)                                      # :102
    try:
        r = gplite_sample_device(gp, Ns, LB, UB, x0=x0, E=E, thin=thin, burnin=burnin, beta=beta, VarThresh=VarThresh, spec=spec,
                                 chunk=chunk, seed=seed, uniforms=uniforms, outputs=("X",), engine=engine)
        Xs = r["X"]
    except VbmcUnsupported as err:
        if "resident" not in str(err):
            raise
        engine = engine or default_engine()
        Nm = -(-Ns // E)
        xs, _ = ensemble_slice_sample(_log_gpfun_host(gp, float(beta), float(VarThresh), engine), x0, Nm, LB, UB, thin=int(thin),
                                      burnin=int(np.ceil(Ns / 5)) if burnin is None else int(burnin), rng=np.random.default_rng(int(seed)))
        Xs, r = np.transpose(xs, (1, 0, 2)).reshape(Nm * E, D)[:Ns], None        # row e + E i: record i of ensemble e
    return (Xs, r) if nargout > 1 else Xs

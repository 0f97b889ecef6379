"""Acquisition sweep on the GPU behind the reference's call surface.

``acqwrapper_vbmc(Xs, vp, gp, optimState, transpose_flag, acqFun, acqInfo)`` (acq/acqwrapper_vbmc.m:1) with the
density-based acquisition functions ``acqf_vbmc`` (default, vbmc.m:213), ``acqflog_vbmc``, ``acqus_vbmc``,
``acqfsn2_vbmc`` and the importance-sampled ``acqviqr_vbmc`` / ``acqimiqr_vbmc`` (noisy targets): GP prediction for every hyper-sample, the hyper-sample statistics, the variational-posterior
density and the acquisition value are one fused device pass (``vbmc_acq_eval``).  The two steps that need VBMC's
variable transform -- the integer mapping (:8) and the hard-bound test in the ORIGINAL space (:49-51) -- are the
caller's: pass the boolean mask of out-of-bounds points as ``outside``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _pack
from ._lib import AcqSearchArgs, IsSampleArgs, IsSetupArgs, VbmcUnsupported, f64, host_dump, new_args, ptr
from .elbo import default_engine
from .ensemble import ensemble_slice_sample
from .gplite import _device_gp_with_noise, gplite_pred_device
from .mixture import vbmc_lnpdf as _vbmc_lnpdf, vbmc_moments, vbmc_rnd
from .optimize import gethpd_vbmc

ACQ_IDS = {"acqf_vbmc": 0, "acqflog_vbmc": 1, "acqus_vbmc": 2, "acqfsn2_vbmc": 3, "acqviqr_vbmc": 10, "acqimiqr_vbmc": 11}


class ImportanceState:
    """Device copy of optimState.ActiveImportanceSampling (vbmc_acq_is_create); freed with the object."""

    @classmethod
    def from_handle(cls, engine, handle):
        """Wrap a state the library built on the device (vbmc_acq_is_sample); owned, and freed, like an uploaded one."""
        self = cls.__new__(cls)
        self.ctx = engine.ctx
        self.h = handle
        return self

    def __init__(self, engine, dgp, ais):
        self.ctx = engine.ctx
        Xa = np.asarray(ais["Xa"], dtype=np.float64)
        per_s = Xa.ndim == 3
        Na = Xa.shape[0]
        xa = f64(Xa.reshape(Na, -1, order="F")) if per_s else f64(Xa)
        lnw = ais.get("lnw")
        lnw = None if lnw is None or np.size(lnw) == 0 else f64(np.asarray(lnw, dtype=np.float64).reshape(dgp.S, Na))
        fs2a = ais.get("fs2a")
        fs2a = None if fs2a is None else f64(np.asarray(fs2a, dtype=np.float64).reshape(Na, dgp.S))
        ct = ais.get("Ctmp_mat")
        ct = None if ct is None else f64(np.asarray(ct, dtype=np.float64).reshape(dgp.N, -1, order="F"))
        self.h = C.c_void_p()
        self.ctx.check(self.ctx.lib.vbmc_acq_is_create(self.ctx.h, dgp.h, Na, ptr(xa), int(per_s), ptr(lnw), ptr(fs2a), ptr(ct),
                                                       C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.vbmc_acq_is_free(self.ctx.h, self.h)
                self.h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def _importance_state(engine, dgp, ais):
    """One-entry cache on the ActiveImportanceSampling dict itself (it is rebuilt once per active-sampling step,
    private/activesample_vbmc.m:209-212, and then reused by every acquisition call of that step)."""
    st = ais.get("_device")
    if st is None or st[0] is not dgp:
        st = (dgp, ImportanceState(engine, dgp, ais))
        ais["_device"] = st
    return st[1]


def acq_info(acqFun):
    """acqFun([]) info struct of the accelerated functions (acq/acqflog_vbmc.m:6-11)."""
    name = acqFun if isinstance(acqFun, str) else getattr(acqFun, "__name__", str(acqFun))
    name = name.lstrip("@")
    if name not in ACQ_IDS:
        raise VbmcUnsupported(-1, "acquisition function %s is not accelerated" % name)
    iqr = name in ("acqviqr_vbmc", "acqimiqr_vbmc")
    info = {"name": name, "log_flag": name == "acqflog_vbmc" or iqr, "compute_varlogjoint": False}
    if iqr:  # acq/acqviqr_vbmc.m:8-11, acq/acqimiqr_vbmc.m:8-10
        info.update(importance_sampling=True, importance_sampling_vp=False, variational_importance_sampling=name == "acqviqr_vbmc")
    return info


def acqwrapper_vbmc(Xs, vp, gp, optimState, transpose_flag=False, acqFun="acqf_vbmc", acqInfo=None, *, outside=None,
                    nargout=1, engine=None, shard=None, delta_quad=False):
    """acq = acqwrapper_vbmc(Xs,vp,gp,optimState,transpose_flag,acqFun,acqInfo).

    ``optimState`` keys used: ymax, VarianceRegularizedAcqFcn, TolGPVar (+ gplengthscale for acqfsn2 / acqviqr /
    acqimiqr, whose gp needs X_rescaled and sn2new, + ActiveImportanceSampling for the IQR functions).
    ``nargout=3`` also returns (fbar, vtot) of :21-29.

    ``delta_quad=True``: with any(vp.delta > 0) the mean and variance per hyper-sample come from the quadrature pass
    gplite_quad(gp,Xs,vp.delta',1) (:12-14) on the device (``vbmc_acq_eval_delta``; the four density-based functions).  The default
    keeps refusing vp.delta > 0 with VbmcUnsupported.

    Sharded form: ``shard`` = (rank, world, allgather) from vbmc_amd.dist.shard_spec() makes every rank evaluate the
    test points i = rank (mod world) on its own GPU (full GP replica) and all-gather the acquisition values, so that
    all ranks hold the identical vector and pick the identical argmin (private/activesample_vbmc.m:227-233)."""
    quad_kw = {"delta_quad": True} if delta_quad else {}
    if shard is not None:
        rank, world, allgather = shard
        X_ = np.asarray(Xs, dtype=np.float64)
        if transpose_flag:
            X_ = X_.T
        X_ = X_.reshape(-1, gp["X"].shape[1])
        n = X_.shape[0]
        idx = np.arange(n)[rank::world]
        out_l = None if outside is None else np.asarray(outside, dtype=bool).reshape(-1)[idx]
        if idx.size:
            loc = _acq_local(X_[idx], vp, gp, optimState, acqFun, out_l, 3, engine, **quad_kw)
        else:
            loc = (np.zeros(0), np.zeros(0), np.zeros(0))
        full = [allgather(v, idx, n) for v in (loc if nargout >= 3 else loc[:1])]
        acq = full[0].reshape(1, -1) if transpose_flag else full[0]
        return (acq, full[1], full[2]) if nargout >= 3 else acq
    return _acq_local(Xs, vp, gp, optimState, acqFun, outside, nargout, engine, transpose_flag, **quad_kw)


def _acq_local(Xs, vp, gp, optimState, acqFun, outside, nargout, engine, transpose_flag=False, delta_quad=False):
    """The single-GPU evaluation behind acqwrapper_vbmc (one fused device pass)."""
    engine = engine or default_engine()
    ctx = engine.ctx
    info = acq_info(acqFun)
    acq_id = ACQ_IDS[info["name"]]
    delta = vp.get("delta")
    use_quad = delta is not None and np.size(delta) > 0 and bool(np.any(np.asarray(delta) > 0))    # :12
    if use_quad and not delta_quad:
        raise VbmcUnsupported(-1, "vp.delta > 0 (gplite_quad, acqwrapper_vbmc.m:12-14) is not accelerated")
    if use_quad and acq_id >= 10:
        raise VbmcUnsupported(-1, "vp.delta > 0 with %s is not accelerated" % info["name"])
    Xs = np.asarray(Xs, dtype=np.float64)
    if transpose_flag:
        Xs = Xs.T
    Xs = f64(Xs.reshape(-1, gp["X"].shape[1]))
    Nstar, D = Xs.shape
    K = int(vp["K"])
    dgp = _device_gp_with_noise(engine, gp)
    mu, sigma, lam, w = _pack.mixture(vp, D=D)
    gl = xr = sn = None
    if acq_id == 3 or acq_id >= 10:
        gl, xr, sn = _pack.nn_noise(None, optimState["gplengthscale"], gp["X_rescaled"], gp["sn2new"], dgp.N, D)
    if acq_id >= 10:
        ist = _importance_state(engine, dgp, optimState["ActiveImportanceSampling"])
        acq = np.zeros(Nstar)
        fbar = np.zeros(Nstar)
        vtot = np.zeros(Nstar)
        ctx.check(ctx.lib.vbmc_acq_iqr_eval(ctx.h, dgp.h, ist.h, Nstar, ptr(Xs), ptr(gl), ptr(xr), ptr(sn),
                                            int(bool(optimState.get("VarianceRegularizedAcqFcn", False))),
                                            float(optimState.get("TolGPVar", 0.0)), ptr(acq), ptr(fbar), ptr(vtot)))
        if outside is not None:
            acq = np.where(np.asarray(outside, dtype=bool).reshape(-1), np.inf, acq)
        if transpose_flag:
            acq = acq.reshape(1, -1)
        return (acq, fbar, vtot) if nargout >= 3 else acq
    acq = np.zeros(Nstar)
    fbar = np.zeros(Nstar)
    vtot = np.zeros(Nstar)
    args = (ctx.h, dgp.h, Nstar, ptr(Xs), acq_id, K, ptr(mu), ptr(sigma), ptr(lam), ptr(w),
            float(optimState.get("ymax", 0.0)), int(bool(optimState.get("VarianceRegularizedAcqFcn", False))),
            float(optimState.get("TolGPVar", 0.0)), ptr(gl), ptr(xr), ptr(sn), ptr(acq), ptr(fbar), ptr(vtot))
    if use_quad:
        ctx.check(ctx.lib.vbmc_acq_eval_delta(*args, ptr(_pack.delta_row(vp, D))))
    else:
        ctx.check(ctx.lib.vbmc_acq_eval(*args))
    if outside is not None:
        acq = np.where(np.asarray(outside, dtype=bool).reshape(-1), np.inf, acq)   # :49-51
    if transpose_flag:
        acq = acq.reshape(1, -1)
    return (acq, fbar, vtot) if nargout >= 3 else acq


_U_IQR = 0.6745   # norminv(0.75), acq/acqviqr_vbmc.m:4, acq/acqimiqr_vbmc.m:4


def _islogf(name, which, vlnpdf, fmu, fs2):
    """acqfun('islogf1' | 'islogf2' | 'islogf', vlnpdf, [], [], fmu, fs2) of the two importance-sampled acquisition functions
    (acq/acqviqr_vbmc.m:13-30, acq/acqimiqr_vbmc.m:12-27): the log base density of the importance sampler, split into the part
    that is fixed per point (1) and the part added per GP hyper-sample (2)."""
    fs = np.sqrt(np.maximum(fs2, np.finfo(np.float64).tiny))     # (a degenerate hyper-sample -- fs2 <= 0 by rounding -- degrades to a tiny
    added = _U_IQR * fs + np.log1p(-np.exp(-2 * _U_IQR * fs))    # density instead of a NaN that aborts the whole set-up)
    if which == "islogf2":
        return added
    fixed = fmu if name == "acqimiqr_vbmc" else (np.zeros_like(fs2) if which == "islogf1" else np.asarray(vlnpdf).reshape(-1, 1))
    return fixed if which == "islogf1" else fixed + added


def _proposal_lnw(Xa, gp, vp_is, w_vp, rect_delta, name, vp, isamplevp, engine):
    """[lnw, fs2] = activesample_proposalpdf(...) (private/activeimportancesampling_vbmc.m:301-340): log importance weights of
    points drawn from the mixture of the smoothed variational posterior and of box-uniforms centred on the training inputs.
    The GP prediction at the points runs on the device; the two proposal densities are O(Na (K + N) D) on the host."""
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    _, _, fmu, fs2 = gplite_pred_device(gp, Xa, engine)
    logs = []
    if w_vp > 0:
        logs.append(_vbmc_lnpdf(vp_is, Xa) + np.log(w_vp))                                            # :313-315
    vln = np.maximum(_vbmc_lnpdf(vp, Xa), np.log(np.finfo(np.float64).tiny)) if isamplevp else None  # :321-323
    lny = _islogf(name, "islogf1", vln, fmu, fs2)
    if w_vp < 1:                                                                                     # :328-336
        VV = np.prod(2 * rect_delta)
        inside = np.all(np.abs(Xa[:, None, :] - X[None, :, :]) < rect_delta[None, None, :], axis=2)   # Na x N
        with np.errstate(divide="ignore"):
            logs.append(np.log(np.sum(inside, axis=1) / VV / N * (1 - w_vp)))
    T = np.stack(logs, axis=1)
    m = np.max(T, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lpdf = (m + np.log(np.sum(np.exp(T - m), axis=1, keepdims=True)))
    return lny - lpdf, fs2                                                                           # Na x S each


def importance_sample_rng_dump(seed, S, H, M):
    """U (64 x H x S x M) that ``importance_sample_device(..., seed=seed)`` consumes (vbmc_acq_is_sample_rng_dump: a pure host function)."""
    U = np.zeros((64, H, S, M), order="F")
    host_dump("vbmc_acq_is_sample_rng_dump", seed, S, H, M, U)
    return U


def importance_sample_device(gp, x0, LB, UB, Nm, *, thin=1, burnin=None, spec=0, seed=0, uniforms=None, chunk=0, max_steps=0,
                             max_shrink=0, engine=None, want_state=True):
    """The thin ctypes call of ``vbmc_acq_is_sample`` (include/vbmc_hip.h): the MCMC of the IMIQR importance sampler, one ensemble of
    W walkers per GP hyper-sample, the whole sampler on the device.  ``x0``: S x W x D starting walkers (as ``ensemble_slice_sample``
    takes them).  ``uniforms`` (64 x H x S x Mmax): parity mode, the library's own generator keyed by ``seed`` otherwise.
    Returns a dict: Xa (Nm x D x S), lnw (S x Nm), fs2a (Nm x S), logp (S x Nm), funccount, performed, rounds, behind and ``state``,
    the ``ImportanceState`` of those device buffers (None without ``want_state``)."""
    engine = engine or default_engine()
    ctx = engine.ctx
    dgp = _device_gp_with_noise(engine, gp)
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 3:
        raise ValueError("importance_sample_device: x0 must be S x W x D")
    S, W, D = x0.shape
    if (S, D) != (len(gp["post"]), np.asarray(gp["X"]).shape[1]):
        raise ValueError("importance_sample_device: x0 is S x W x D = %d x %d x %d, the GP has S = %d hyper-samples and D = %d"
                         % (S, W, D, len(gp["post"]), np.asarray(gp["X"]).shape[1]))
    Nm = int(Nm)
    keep = [f64(np.transpose(x0, (1, 2, 0))), *_pack.box(LB, UB, D)]      # x0: W x D x S
    a = new_args(IsSampleArgs)
    a.D, a.S = int(D), int(S)
    _pack.sampler_opts(a, W, Nm, thin, burnin, spec, max_steps, max_shrink, chunk, seed)
    a.x0, a.LB, a.UB = (ptr(k) for k in keep)
    if uniforms is not None:
        keep.append(_pack.sampler_uniforms(a, uniforms, W // 2, S, "importance_sample_device"))
        a.rng_mode = 1
    n = max(Nm, 1)
    out = {"Xa": np.zeros((n, D, S), order="F"), "lnw": np.zeros((S, n), order="F"), "fs2a": np.zeros((n, S), order="F"),
           "logp": np.zeros((S, n), order="F")}
    handle = C.c_void_p()
    a.Xa, a.lnw, a.fs2a, a.logp = ptr(out["Xa"]), ptr(out["lnw"]), ptr(out["fs2a"]), ptr(out["logp"])
    counts = _pack.counters(a)
    if want_state:
        a.state = C.pointer(handle)
    ctx.check(ctx.lib.vbmc_acq_is_sample(ctx.h, dgp.h, C.byref(a)))
    out.update(counts(), state=ImportanceState.from_handle(engine, handle) if want_state else None, _dgp=dgp)
    return out


def importance_setup_rng_dump(seed, D, S, W, Nvp, Nbox):
    """The block B ((D + 1) (Nvp + Nbox) + W S doubles) that ``importance_setup_device(..., seed=seed)`` consumes in Step 1 and in the
    resampling (vbmc_acq_is_setup_rng_dump: a pure host function)."""
    B = np.zeros((D + 1) * (Nvp + Nbox) + W * S)
    host_dump("vbmc_acq_is_setup_rng_dump", seed, D, S, W, Nvp, Nbox, B)
    return B


def importance_setup_device(vp, gp, Nvp, Nbox, Nm, *, W=None, thin=1, burnin=None, spec=0, seed=0, block=None, uniforms=None, chunk=0,
                            max_steps=0, max_shrink=0, engine=None, want_state=True):
    """The thin ctypes call of ``vbmc_acq_is_setup`` (include/vbmc_hip.h): Step 1 of the IMIQR importance sampler, the resampling of
    the starting walkers, the MCMC, the closing prediction and the importance-sampling state in one call.  ``block``: the caller's
    Step 1 block (parity mode; ``uniforms``, 64 x H x S x Mmax, is then Step 2's, optional), the library's generator keyed by ``seed``
    otherwise.  ``Nm = 0``: Step 1 alone.  Returns a dict: Xa1 (Na1 x D), lnw1 (S x Na1), fs2a1 (Na1 x S), lpdf1 (Na1), rect_delta, LB,
    UB, and with Nm > 0 x0 (S x W x D, as ``importance_sample_device`` takes them), idx0 (W x S), n_bad, bad (W x S) and -- unless
    n_bad > 0 -- what ``importance_sample_device`` returns."""
    engine = engine or default_engine()
    ctx = engine.ctx
    dgp = _device_gp_with_noise(engine, gp)
    D, K, S = int(vp["D"]), int(vp["K"]), len(gp["post"])
    Nvp, Nbox, Nm = int(Nvp), int(Nbox), int(Nm)
    W = 2 * (D + 1) if W is None else int(W)
    Na1 = max(Nvp + Nbox, 1)
    a = new_args(IsSetupArgs)
    a.D, a.S, a.K, a.Nvp, a.Nbox = D, S, K, Nvp, Nbox
    keep = list(_pack.mixture(vp, a))
    _pack.sampler_opts(a, W, Nm, thin, burnin, spec, max_steps, max_shrink, chunk, seed)
    if block is not None:
        B = f64(np.asarray(block, dtype=np.float64).reshape(-1))
        if B.size != (D + 1) * (Nvp + Nbox) + (W * S if Nm > 0 else 0):
            raise ValueError("importance_setup_device: the block must hold (D + 1) (Nvp + Nbox) + W S values")
        a.rng_mode, a.B = 1, ptr(B)
        keep.append(B)
        if uniforms is not None:
            keep.append(_pack.sampler_uniforms(a, uniforms, W // 2, S, "importance_setup_device"))
    elif uniforms is not None:
        raise ValueError("importance_setup_device: uniforms (Step 2's block) go with a Step 1 block")
    n, w = max(Nm, 1), max(W, 1)
    out = {"Xa1": np.zeros((Na1, D), order="F"), "lnw1": np.zeros((S, Na1), order="F"), "fs2a1": np.zeros((Na1, S), order="F"),
           "lpdf1": np.zeros(Na1), "rect_delta": np.zeros(D), "LB": np.zeros(D), "UB": np.zeros(D)}
    x0 = np.zeros((w, D, S), order="F")
    idx0 = np.zeros((w, S), dtype=np.int32, order="F")
    bad = np.zeros((w, S), dtype=np.uint8, order="F")
    run = {"Xa": np.zeros((n, D, S), order="F"), "lnw": np.zeros((S, n), order="F"), "fs2a": np.zeros((n, S), order="F"),
           "logp": np.zeros((S, n), order="F")}
    nb = C.c_int32()
    handle = C.c_void_p()
    a.Xa1, a.lnw1, a.fs2a1, a.lpdf1 = ptr(out["Xa1"]), ptr(out["lnw1"]), ptr(out["fs2a1"]), ptr(out["lpdf1"])
    a.rect_delta, a.LB, a.UB, a.x0 = ptr(out["rect_delta"]), ptr(out["LB"]), ptr(out["UB"]), ptr(x0)
    a.idx0 = idx0.ctypes.data_as(_pack.i32p)
    a.bad = bad.ctypes.data_as(C.POINTER(C.c_uint8))
    a.n_bad = C.pointer(nb)
    a.Xa, a.lnw, a.fs2a, a.logp = ptr(run["Xa"]), ptr(run["lnw"]), ptr(run["fs2a"]), ptr(run["logp"])
    counts = _pack.counters(a)
    if want_state:
        a.state = C.pointer(handle)
    ctx.check(ctx.lib.vbmc_acq_is_setup(ctx.h, dgp.h, C.byref(a)))
    out.update(counts(), n_bad=int(nb.value), _dgp=dgp,
               state=ImportanceState.from_handle(engine, handle) if want_state and handle.value else None)
    if Nm > 0:
        out.update(x0=np.ascontiguousarray(np.transpose(x0, (2, 0, 1))), idx0=idx0, bad=bad.astype(bool))
        if out["n_bad"] == 0:
            out.update(run)
    return out


def _patch_starts(x0, bad, X, LB, UB, logp, rng):
    """Replace the starting walkers flagged in ``bad`` (S x W) by training inputs inside the box at which the target is finite."""
    inside = X[np.all((X >= LB) & (X <= UB), axis=1)]
    for s, i in zip(*np.nonzero(bad)):
        for cand in inside[rng.permutation(inside.shape[0])[:16]]:
            if np.isfinite(logp(cand[None, :], np.array([s]))[0]):
                x0[s, i] = cand
                break


def _importance_setup_one_call(vp, gp, Nvp, Nbox, Nm, thin, rng, seed, engine):
    """The IMIQR set-up through ``importance_setup_device``; None where the library answers 'unsupported'."""
    if Nvp + Nbox > 256:                                        # more Step 1 points than an importance-sampling state holds (max_Na)
        return None
    sd = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
    try:
        r = importance_setup_device(vp, gp, Nvp, Nbox, max(Nm, 0), thin=thin, seed=sd, engine=engine)
    except VbmcUnsupported:
        return None
    if Nm <= 0:
        return {"Xa": r["Xa1"], "lnw": r["lnw1"], "fs2a": r["fs2a1"], "_device": (r["_dgp"], r["state"])}
    if r["n_bad"] > 0:
        X = np.asarray(gp["X"], dtype=np.float64)

        def logp(P, e):
            fm, f2, _, _ = gplite_pred_device(gp, P, engine)
            k = np.arange(P.shape[0])
            v = _islogf("acqimiqr_vbmc", "islogf", None, fm[k, e].reshape(-1, 1), f2[k, e].reshape(-1, 1)).reshape(-1)
            return np.where(np.isfinite(v), v, -np.inf)

        x0 = r["x0"].copy()
        _patch_starts(x0, r["bad"].T, X, r["LB"], r["UB"], logp, rng)
        try:
            r = importance_sample_device(gp, x0, r["LB"], r["UB"], Nm, thin=thin, seed=sd, engine=engine)
        except VbmcUnsupported:
            return None
    return {"Xa": r["Xa"], "lnw": r["lnw"], "fs2a": r["fs2a"], "logp": r["logp"], "funccount": r["funccount"], "performed": r["performed"],
            "rounds": r["rounds"], "_device": (r["_dgp"], r["state"])}


def activeimportancesampling_vbmc(vp, gp, acqFun, acqInfo=None, options=None, *, rng=None, engine=None, device=False, seed=None,
                                  one_call=True):
    """ActiveImportanceSampling = activeimportancesampling_vbmc(vp,gp,acqfun,acqinfo,options)
    (private/activeimportancesampling_vbmc.m).

    acqviqr_vbmc (variational_importance_sampling, :36-52,92-100): Na draws from the variational posterior, lnw = 0.
    acqimiqr_vbmc (round 3; :103-246): importance sampling-resampling from the smoothed variational posterior and box-uniforms
    around the training inputs (Step 1), then, per GP hyper-sample, MCMC on the log base density fmu + u fs + log1p(-exp(-2 u fs))
    started from a weighted resample of those points (Step 2) -- all hyper-samples' ensembles advance together, every
    log-density evaluation is one batched GP prediction on the device (the reference predicts one point at a time,
    log_isbasefun :343-353), the transition operator is ensemble_slice_sample above.  Xa is then Na x D x S and lnw S x Na.
    Step 3 (fs2a, Kax, Ctmp) happens on the device inside vbmc_acq_is_create at the first acquisition call.

    ``device=True`` (acqimiqr_vbmc without importance_sampling_vp): Step 2 runs on the device (``importance_sample_device``), and with
    ``one_call`` the whole set-up does (``importance_setup_device``: Step 1, the resampling, Step 2 and the state in one call; the
    random numbers are then the library's, keyed by ``seed`` or by one draw from ``rng``).  Starting walkers of zero density are patched
    on the host as below and handed to ``importance_sample_device``; an unsupported GP falls back to the path without the one call."""
    info = acqInfo or acq_info(acqFun)
    name = info.get("name") or (acqFun if isinstance(acqFun, str) else acqFun.__name__).lstrip("@")
    engine = engine or default_engine()
    rng = np.random.default_rng(0) if rng is None else rng
    opts = dict(options or {})
    K, D = int(vp["K"]), int(vp["D"])

    def evalopt(v, default):
        v = opts.get(v, default)
        return int(np.ceil(v(K, D) if callable(v) else v))

    S = len(gp["post"])
    if info.get("variational_importance_sampling", False):
        Na = evalopt("ActiveImportanceSamplingMCMCSamples", 100)          # vbmc.m:337 default '100'
        if Na <= 0:
            raise ValueError("OPTIONS.ActiveImportanceSamplingMCMCSamples should be (or evaluate to) a positive integer.")
        Xa, _ = vbmc_rnd(vp, Na, False, rng=rng)
        return {"Xa": Xa, "lnw": np.zeros((S, Na))}        # fs2a / Ctmp_mat are produced on the device from Xa
    if delta_positive(vp):
        raise VbmcUnsupported(-1, "vp.delta > 0 is not accelerated")
    isamplevp = bool(info.get("importance_sampling_vp", False))
    X = np.asarray(gp["X"], dtype=np.float64)
    # ---- Step 1: importance sampling-resampling (:103-151)
    Nvp = evalopt("ActiveImportanceSamplingVPSamples", 100)
    Nbox = evalopt("ActiveImportanceSamplingBoxSamples", 100)
    if Nvp + Nbox <= 0:
        raise ValueError("activeimportancesampling_vbmc: no importance samples requested")
    on_device = device and name == "acqimiqr_vbmc" and not isamplevp      # (the device target is IMIQR's log base density and nothing else)
    if on_device and one_call:
        r = _importance_setup_one_call(vp, gp, Nvp, Nbox, evalopt("ActiveImportanceSamplingMCMCSamples", 100),
                                       max(1, evalopt("ActiveImportanceSamplingMCMCThin", 1)), rng, seed, engine)
        if r is not None:
            return r
    w_vp = Nvp / (Nvp + Nbox)
    rect_delta = 2 * np.std(X, axis=0, ddof=1)
    lnw_l, Xa_l, fs2_l = [], [], []
    vp_is = None
    if Nvp > 0:
        mu = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)
        sig = np.asarray(vp["sigma"], dtype=np.float64).reshape(K)
        w = np.asarray(vp["w"], dtype=np.float64).reshape(K)
        sc = (0.05, 0.2, 1.0)                                                                        # :114
        vp_is = dict(vp, K=K * (1 + len(sc)), w=np.tile(w, 1 + len(sc)) / (1 + len(sc)), mu=np.tile(mu, (1, 1 + len(sc))),
                     sigma=np.concatenate([sig] + [np.sqrt(sig ** 2 + c * c) for c in sc]))
        Xv, _ = vbmc_rnd(vp_is, Nvp, False, rng=rng)
        lw, f2 = _proposal_lnw(Xv, gp, vp_is, w_vp, rect_delta, name, vp, isamplevp, engine)
        lnw_l.append(lw); Xa_l.append(Xv); fs2_l.append(f2)
    if Nbox > 0:
        jj = rng.integers(0, X.shape[0], size=Nbox)
        Xb = X[jj] + (2 * rng.random((Nbox, D)) - 1) * rect_delta[None, :]                            # :138-139
        lw, f2 = _proposal_lnw(Xb, gp, vp_is, w_vp, rect_delta, name, vp, isamplevp, engine)
        lnw_l.append(lw); Xa_l.append(Xb); fs2_l.append(f2)
    Xa1 = np.concatenate(Xa_l, axis=0)
    lnw1 = np.concatenate(lnw_l, axis=0).T                    # S x Na
    lnw1 = np.where(np.isfinite(lnw1), lnw1, -np.inf)          # :146
    fs2a1 = np.concatenate(fs2_l, axis=0)
    Nm = evalopt("ActiveImportanceSamplingMCMCSamples", 100)
    if Nm <= 0:
        return {"Xa": Xa1, "lnw": lnw1, "fs2a": fs2a1}
    # ---- Step 2: MCMC per GP hyper-sample (:155-246), all S ensembles in lock-step
    thin = max(1, evalopt("ActiveImportanceSamplingMCMCThin", 1))
    burnin = int(np.ceil(thin * Nm / 2))
    W = 2 * (D + 1)
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    LB = np.min(X, axis=0) - 0.5 * diam                                                              # :25-28
    UB = np.max(X, axis=0) + 0.5 * diam
    _, _, fmu1, fs21 = gplite_pred_device(gp, Xa1, engine)
    x0 = np.empty((S, W, D))
    for s in range(S):                                                                                # :196-205 resampling without replacement
        lw = lnw1[s] + _islogf(name, "islogf2", None, fmu1[:, s:s + 1], fs21[:, s:s + 1]).reshape(-1)
        ww = np.exp(lw - np.max(lw))
        for i in range(W):
            if not np.sum(ww) > 0:
                ww = np.ones_like(ww)
            idx = int(np.searchsorted(np.cumsum(ww), rng.random() * np.sum(ww), side="right"))         # catrnd (:385-410)
            idx = min(idx, ww.size - 1)
            ww[idx] = 0.0
            x0[s, i] = np.clip(Xa1[idx], LB, UB)

    def logp(P, e):                                                                                   # log_isbasefun :343-353
        # (:346 reads the FIRST two outputs of gplite_pred -- ymu, ys2: the predictive variance with the observation noise -- not the
        # latent fmu, fs2 the proposals above use)
        fm, f2, _, _ = gplite_pred_device(gp, P, engine)
        r = np.arange(P.shape[0])
        vln = np.maximum(_vbmc_lnpdf(vp, P), np.log(np.finfo(np.float64).tiny)) if isamplevp else None
        v = _islogf(name, "islogf", vln, fm[r, e].reshape(-1, 1), f2[r, e].reshape(-1, 1)).reshape(-1)
        return np.where(np.isfinite(v), v, -np.inf)

    # a walker that starts at zero density (a clipped point, a duplicate drawn after the weights ran out) is replaced by a training input
    # inside the box -- the sampler would refuse it, and one degenerate hyper-sample must not abort the acquisition set-up
    lp0 = logp(x0.reshape(S * W, D), np.repeat(np.arange(S), W)).reshape(S, W)
    _patch_starts(x0, ~np.isfinite(lp0), X, LB, UB, logp, rng)
    if on_device:
        try:
            sd = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
            r = importance_sample_device(gp, x0, LB, UB, Nm, thin=thin, burnin=burnin, seed=sd, engine=engine)
            return {"Xa": r["Xa"], "lnw": r["lnw"], "fs2a": r["fs2a"], "logp": r["logp"], "funccount": r["funccount"], "performed": r["performed"],
                    "rounds": r["rounds"], "_device": (r["_dgp"], r["state"])}
        except VbmcUnsupported:
            pass                                                  # beyond the device sampler's range: the host-driven one below
    Xs, lps, info_s = ensemble_slice_sample(logp, x0, Nm, LB, UB, thin=thin, burnin=burnin, rng=rng, return_info=True)
    Xa = np.transpose(Xs, (1, 2, 0)).copy()                       # Na x D x S
    lnw = np.empty((S, Nm))
    fs2a = np.empty((Nm, S))
    _, _, fm_all, f2_all = gplite_pred_device(gp, Xs.reshape(S * Nm, D), engine)
    for s in range(S):                                            # :209-221: lnw = islogf1 - log p of the chain's target
        fm = fm_all[s * Nm:(s + 1) * Nm, s:s + 1]
        f2 = f2_all[s * Nm:(s + 1) * Nm, s:s + 1]
        vln = np.maximum(_vbmc_lnpdf(vp, Xs[s]), np.log(np.finfo(np.float64).tiny)) if isamplevp else None
        lnw[s] = _islogf(name, "islogf1", vln, fm, f2).reshape(-1) - lps[s]
        fs2a[:, s] = f2.reshape(-1)
    return {"Xa": Xa, "lnw": lnw, "fs2a": fs2a, "funccount": info_s["funccount"]}


# ------------------------------------------------------------------------------------------
# The acquisition search of active sampling on the device (vbmc_acq_search)
SEARCH_STOP = {1: "TolX", 2: "TolFun", 3: "TolHistFun", 4: "MaxFunEvals", 5: "MaxIter"}


def acq_search_rng_dump(seed, D, lam, G):
    """Z (D x lam x G) that ``acq_search(..., seed=seed)`` consumes (vbmc_acq_search_rng_dump: a pure host function)."""
    Z = np.zeros((D, lam, G), order="F")
    host_dump("vbmc_acq_search_rng_dump", seed, D, lam, G, Z)
    return Z


def acq_search(x0, insigma, LB, UB, vp, gp, optimState, acqFun="acqf_vbmc", *, TolX, TolFun, TolHistFun, MaxFunEvals=0, MaxIter=0,
               popsize=0, seed=0, Z=None, chunk=0, trace=0, engine=None, iqr=None):
    """The thin ctypes call of ``vbmc_acq_search`` (include/vbmc_hip.h): CMA-ES in its Cholesky form on ``acqwrapper_vbmc`` inside
    the box [LB, UB], started at ``x0`` with the coordinate-wise standard deviations ``insigma``, the whole optimiser on the device.
    ``acqFun``: a name, or the library's numeric id (what the library does not take it refuses itself).
    The IQR functions (``acqviqr_vbmc`` / ``acqimiqr_vbmc``, ids 10 / 11) with ``optimState["ActiveImportanceSampling"]`` present go to
    ``vbmc_acq_search_iqr`` on the device copy of that state (built or reused as ``acqwrapper_vbmc`` does); without the state the call
    reaches ``vbmc_acq_search``, which refuses them.  ``iqr`` = True / False forces the entry point (tests of the library's refusals).
    ``Z`` (D x lam x Gmax normals): parity mode, the library's own generator keyed by ``seed`` otherwise.  ``trace`` = n keeps the
    rank order, the sorted values, xmean and sigma of the first n generations.  Returns a dict: xmin / fmin (the last generation's
    best), xbest / fbest (the best ever seen), xmean, sigma, C, evals, generations, stop (name), behind (launches enqueued behind
    the end) and, with ``trace``, tr_order / tr_F / tr_xmean / tr_sigma."""
    engine = engine or default_engine()
    ctx = engine.ctx
    acq_id = int(acqFun) if isinstance(acqFun, (int, np.integer)) else ACQ_IDS[acq_info(acqFun)["name"]]   # a name, or the library's id
    D = gp["X"].shape[1]
    K = int(vp["K"])
    dgp = _device_gp_with_noise(engine, gp)
    a = new_args(AcqSearchArgs)
    a.acq_id, a.K = acq_id, K
    keep = [*_pack.mixture(vp, a, D=D), _pack.delta_row(vp, D), f64(np.asarray(x0, dtype=np.float64).reshape(D)), _pack.row(insigma, D),
            *_pack.box(LB, UB, D)]
    a.vp_delta, a.x0, a.insigma, a.LB, a.UB = (ptr(k) for k in keep[4:])
    a.ymax = float(optimState.get("ymax", 0.0))
    a.var_regularized = int(bool(optimState.get("VarianceRegularizedAcqFcn", False)))
    a.TolGPVar = float(optimState.get("TolGPVar", 0.0))
    ais = optimState.get("ActiveImportanceSampling")
    if iqr is None:
        iqr = acq_id in (10, 11) and ais is not None
    if acq_id == 3 or iqr:                                  # (what is missing stays NULL: the library names it in its refusal)
        both = gp.get("X_rescaled") is not None and gp.get("sn2new") is not None
        keep += _pack.nn_noise(a, optimState.get("gplengthscale"), gp["X_rescaled"] if both else None, gp["sn2new"] if both else None,
                               dgp.N, D)
    a.TolX, a.TolFun, a.TolHistFun = float(TolX), float(TolFun), float(TolHistFun)
    a.MaxFunEvals = 0 if (MaxFunEvals is None or not np.isfinite(MaxFunEvals)) else int(MaxFunEvals)
    a.MaxIter, a.popsize, a.chunk = int(MaxIter or 0), int(popsize or 0), int(chunk or 0)
    lam = int(popsize) if popsize else 4 + int(np.floor(3 * np.log(D)))
    if Z is not None:
        Z = f64(np.asarray(Z, dtype=np.float64))
        if Z.ndim != 3 or Z.shape[:2] != (D, lam):
            raise ValueError("acq_search: Z must be D x lam x Gmax = %d x %d x Gmax" % (D, lam))
        a.rng_mode, a.Gmax, a.Z = 1, Z.shape[2], ptr(Z)
    else:
        a.rng_mode, a.seed = 0, int(seed)
    out = {"xmin": np.zeros(D), "xbest": np.zeros(D), "xmean": np.zeros(D), "C": np.zeros((D, D), order="F")}
    sc = {k: C.c_double() for k in ("fmin", "fbest", "sigma")}
    evals, rounds = C.c_int64(), (C.c_int64 * 2)()
    gens, stop = C.c_int32(), C.c_int32()
    a.xmin, a.xbest, a.xmean, a.C = ptr(out["xmin"]), ptr(out["xbest"]), ptr(out["xmean"]), ptr(out["C"])
    a.fmin, a.fbest, a.sigma = C.pointer(sc["fmin"]), C.pointer(sc["fbest"]), C.pointer(sc["sigma"])
    a.evals, a.generations, a.stop = C.pointer(evals), C.pointer(gens), C.pointer(stop)
    a.rounds = C.cast(rounds, _pack.i64p)
    n = int(trace or 0)
    if n > 0:
        out.update(tr_order=np.zeros((lam, n), dtype=np.int32, order="F"), tr_F=np.zeros((lam, n), order="F"),
                   tr_xmean=np.zeros((D, n), order="F"), tr_sigma=np.zeros(n))
        a.trace_cap = n
        a.tr_order = out["tr_order"].ctypes.data_as(_pack.i32p)
        a.tr_F, a.tr_xmean, a.tr_sigma = ptr(out["tr_F"]), ptr(out["tr_xmean"]), ptr(out["tr_sigma"])
    if iqr:
        ist = _importance_state(engine, dgp, ais)
        ctx.check(ctx.lib.vbmc_acq_search_iqr(ctx.h, dgp.h, ist.h, C.byref(a)))
    else:
        ctx.check(ctx.lib.vbmc_acq_search(ctx.h, dgp.h, C.byref(a)))
    out.update(fmin=sc["fmin"].value, fbest=sc["fbest"].value, sigma=sc["sigma"].value, evals=int(evals.value),
               generations=int(gens.value), stop=SEARCH_STOP.get(int(stop.value), "MaxIter"), behind=int(rounds[1]), popsize=lam)
    return out


SEARCH_DEFAULT_OPTIONS = {
    "SearchOptimizer": "cmaes", "SearchCMAESVPInit": True, "SearchCMAESbest": False, "SearchMaxFunEvals": None, "HPDFrac": 0.8,
    # misc/setupoptions_vbmc.m:168-170
    "CMAESopts": {"TolX": lambda insigma: 1e-11 * float(np.max(insigma)), "TolHistFun": 1e-13},
}


def active_search(Xsearch, vp, gp, optimState, options=None, acqFun="acqf_vbmc", *, outside=None, seed=0, engine=None, info=None):
    """The search for ONE new point of private/activesample_vbmc.m:227-329: the acquisition sweep over ``Xsearch`` and its argmin x0
    (:228-238), the box (:249-255: optimState.LB_search / UB_search widened to hold x0, or the training inputs' range + 10 %), TolFun
    (:257-262), insigma from vbmc_moments (SearchCMAESVPInit, :268,275) or the covariance of the HPD training inputs (:272-273), CMA-ES on
    the device (``acq_search``), SearchCMAESbest (:285-288) and the acceptance test fval_optim < fval_old (:324).

    Returns (Xacq (D,), fval, info) with info = {"x0", "fval_old", "accepted", "search": acq_search's dict or None, "idx"}.  Integer
    variables (real2int_vbmc, :219,248,325) and the hard-bound mask in the original space are the caller's: ``outside`` marks sweep
    points outside the hard bounds, optimState.integervars must be empty."""
    opts = dict(SEARCH_DEFAULT_OPTIONS, **(options or {}))
    iv = optimState.get("integervars")
    if iv is not None and np.any(np.asarray(iv)):
        raise VbmcUnsupported(-1, "active_search: integer variables (real2int_vbmc) are the caller's side")
    engine = engine or default_engine()
    X = np.asarray(gp["X"], dtype=np.float64)
    D = X.shape[1]
    Xsearch = np.asarray(Xsearch, dtype=np.float64).reshape(-1, D)
    acq_fast = acqwrapper_vbmc(Xsearch, vp, gp, optimState, False, acqFun, outside=outside, engine=engine)       # :228
    idx = int(np.argmin(acq_fast))       # :230-236 (the first minimum either way; optimState.SearchCache of :232 is the caller's to keep)
    x0 = Xsearch[idx].copy()
    res = {"x0": x0, "idx": idx, "accepted": False, "search": None}
    if str(opts["SearchOptimizer"]).lower() == "none":                                                    # :246
        res["fval_old"] = float(acq_fast[idx])
        return x0, float(acq_fast[idx]), res
    if str(opts["SearchOptimizer"]).lower() != "cmaes":
        raise VbmcUnsupported(-1, "active_search: SearchOptimizer '%s' is not accelerated ('cmaes' is)" % opts["SearchOptimizer"])
    fval_old = float(acqwrapper_vbmc(x0[None, :], vp, gp, optimState, False, acqFun, engine=engine)[0])   # :247
    res["fval_old"] = fval_old
    lbs, ubs = optimState.get("LB_search"), optimState.get("UB_search")
    if lbs is not None and ubs is not None and np.all(np.isfinite(lbs)) and np.all(np.isfinite(ubs)):     # :249-251
        LB = np.minimum(x0, np.asarray(lbs, dtype=np.float64).reshape(D))
        UB = np.maximum(x0, np.asarray(ubs, dtype=np.float64).reshape(D))
    else:                                                                                                 # :253-254
        xrange = np.max(X, axis=0) - np.min(X, axis=0)
        LB = np.minimum(np.min(X, axis=0), x0) - 0.1 * xrange
        UB = np.maximum(np.max(X, axis=0), x0) + 0.1 * xrange
    info = info or acq_info(acqFun)
    TolFun = 1e-2 if info.get("log_flag") else max(1e-12, abs(fval_old * 1e-3))                           # :257-262
    if opts["SearchCMAESVPInit"]:
        _, Sigma = vbmc_moments(vp, False)                                                                # :268
    else:
        X_hpd, _ = gethpd_vbmc(X, gp["y"], opts["HPDFrac"])                                               # :272-273
        Sigma = np.cov(X_hpd, rowvar=False, bias=True).reshape(D, D)
    insigma = np.sqrt(np.diag(Sigma))                                                                     # :275
    co = dict(SEARCH_DEFAULT_OPTIONS["CMAESopts"], **(opts.get("CMAESopts") or {}))
    TolX = co["TolX"](insigma) if callable(co["TolX"]) else float(co["TolX"])
    maxfe = opts["SearchMaxFunEvals"]
    maxfe = 500 * (D + 2) if maxfe is None else int(maxfe(D) if callable(maxfe) else maxfe)               # vbmc.m:283
    sr = acq_search(x0, insigma, LB, UB, vp, gp, optimState, acqFun, TolX=TolX, TolFun=TolFun, TolHistFun=float(co["TolHistFun"]),
                    MaxFunEvals=maxfe, popsize=int(co.get("PopSize") or 0), seed=seed, engine=engine)
    res["search"] = sr
    x_opt, f_opt = (sr["xbest"], sr["fbest"]) if opts["SearchCMAESbest"] else (sr["xmin"], sr["fmin"])    # :285-288
    if f_opt < fval_old:                                                                                  # :324
        res["accepted"] = True
        return np.asarray(x_opt, dtype=np.float64).copy(), float(f_opt), res
    return x0, fval_old, res


def delta_positive(vp):
    d = vp.get("delta")
    return d is not None and bool(np.any(np.asarray(d) > 0))

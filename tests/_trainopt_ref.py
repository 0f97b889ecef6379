"""NumPy restatement of the optimisation half of gplite_train as this library runs it (include/vbmc_hip.h, vbmc_gp_train_optimize):
the fill stage's bookkeeping (utils/fminfill.m:101-114, gplite/gplite_train.m:206-221,258-272), the library's own projected-BFGS
optimiser, and the closing (:298-306).  The objective is a callable ``fun(x) -> (f, g)``; nothing here touches a device.  It is the
contract of trainopt_kernels.h: the same decisions in the same order, one candidate at a time (the sequential algorithm that
every speculation width W of the device reproduces)."""
import numpy as np

MAXBACK = 30
C1 = 1e-4
EXIT_LIMIT, EXIT_GRAD, EXIT_DF, EXIT_STEP, EXIT_LINESEARCH, EXIT_START = 0, 1, 2, 3, -2, -3


def matlab_eps(x):
    """eps(x) of MATLAB: NaN for an infinite x"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.spacing(x), np.nan)


def clamp_in(x, LB, UB):
    """min(UB - eps(UB), max(LB + eps(LB), x)) with MATLAB's min / max, which pass over NaN (:272,304)"""
    x = np.array(x, dtype=np.float64)
    lo, hi = LB + matlab_eps(LB), UB - matlab_eps(UB)
    x = np.where(np.isnan(lo), x, np.maximum(lo, x))
    return np.where(np.isnan(hi), x, np.minimum(hi, x))


def matlab_sort(v):
    """[sorted, order] = sort(v, 'ascend'): stable, NaN last; order 0-based"""
    v = np.asarray(v, dtype=np.float64)
    key = np.where(np.isnan(v), np.inf, v)
    order = np.lexsort((np.arange(v.size), key, np.isnan(v)))
    return v[order], order


def select_starts(design, fvals, Nopts, Ncov, Nnoise, LB, UB):
    """(fill_fvals, fill_order, starts Nopts x Nhyp, widths_default) from the fill values of the Ninit rows of ``design``"""
    design = np.asarray(design, dtype=np.float64)
    Ninit, Nhyp = design.shape
    fs, order = matlab_sort(fvals)
    Xs = design[order]
    hyp = Xs[:Nopts].copy()                                             # :206
    widths = np.std(design, axis=0, ddof=1) if Ninit > 1 else np.zeros(Nhyp)   # :207
    if Nnoise > 0 and Nopts > 1 and Ninit > Nopts:                      # :210-221
        xx, ny = Xs[Nopts:], fs[Nopts:]
        _, o2 = matlab_sort(xx[:, Ncov])
        xx, ny = xx[o2], ny[o2]
        m20 = int(np.ceil(0.2 * float(ny.size)))
        head = ny[:m20]
        idx = 0 if np.all(np.isnan(head)) else int(np.nanargmin(head))
        hyp[1] = xx[idx]
    z = widths == 0                                                     # :258-267
    if np.any(z) and Nopts > 1:
        widths[z] = np.std(hyp, axis=0, ddof=1)[z]
    z = widths == 0
    if np.any(z):
        widths[z] = np.minimum(1.0, UB[z] - LB[z])
    hyp = np.array([clamp_in(h, LB, UB) for h in hyp])                  # :272
    fixed = LB == UB
    hyp[:, fixed] = LB[fixed]
    return fs, order.astype(np.int32), hyp, widths


def pbfgs(fun, x0, LB, UB, TolFun, MaxIter=1000, MaxFunEvals=3000, margin=None):
    """The projected BFGS of vbmc_gp_train_optimize for ONE start.  Returns a dict: x, f, iterations, funccount, exitflag,
    hist_x, hist_f, hist_k (the accepted backtracking index per iteration).  ``margin``: a list that receives, for every Armijo
    and stopping decision taken, its relative distance from flipping (test-case selection)."""
    LB, UB = np.asarray(LB, dtype=np.float64), np.asarray(UB, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    n = x.size
    fixed = LB == UB
    clip = lambda v: np.minimum(np.maximum(v, LB), UB)
    out = dict(hist_x=[], hist_f=[], hist_k=[])

    def note(lhs, rhs):
        if margin is not None and np.isfinite(lhs) and np.isfinite(rhs):
            margin.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300))

    def finish(flag):
        out.update(x=x, f=f, iterations=it, funccount=fc, exitflag=flag)
        return out

    f, g = fun(x)
    g = np.asarray(g, dtype=np.float64)
    fc, it, fresh = 1, 0, True
    H = np.eye(n)
    if not np.isfinite(f):
        return finish(EXIT_START)
    moved, fold = False, 0.0
    while True:
        pg = np.max(np.abs(x - clip(x - g))) if n else 0.0
        note(pg, TolFun)
        if pg <= TolFun:
            return finish(EXIT_GRAD)
        if moved:
            note(abs(f - fold), TolFun * (1.0 + abs(f)))
            if abs(f - fold) <= TolFun * (1.0 + abs(f)):
                return finish(EXIT_DF)
        if it >= MaxIter or fc >= MaxFunEvals:
            return finish(EXIT_LIMIT)
        free = ~fixed & ~((x <= LB) & (g > 0)) & ~((x >= UB) & (g < 0))
        gF = np.where(free, g, 0.0)
        if not fresh:
            d = np.where(free, -(H @ gF), 0.0)
            if not (g @ d < 0.0):
                fresh = True
        if fresh:
            d = -gF
            t0 = min(1.0, 1.0 / np.sum(np.abs(gF)))
        else:
            t0 = 1.0
        k, accepted = 0, False
        while True:
            if k >= MAXBACK:
                return finish(EXIT_LINESEARCH)
            xc = clip(x + np.ldexp(t0, -k) * d)
            if np.all(xc == x):
                return finish(EXIT_STEP)
            if fc >= MaxFunEvals:
                return finish(EXIT_LIMIT)
            fcand, gc = fun(xc)
            fc += 1
            slope = g @ (xc - x)
            if np.isfinite(fcand):
                note(fcand - f, C1 * slope)
            if np.isfinite(fcand) and fcand <= f + C1 * slope:
                break
            k += 1
        gc = np.asarray(gc, dtype=np.float64)
        s, y = xc - x, np.where(fixed, 0.0, gc - g)
        sy, yy, ss = s @ y, y @ y, s @ s
        if sy > 1e-10 * np.sqrt(ss) * np.sqrt(yy):
            if fresh:
                H = (sy / yy) * np.eye(n)
                fresh = False
            Hy = H @ y
            rho = 1.0 / sy
            H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + (rho * rho * (y @ Hy) + rho) * np.outer(s, s)
        x, fold, f, g = xc, f, fcand, gc
        it += 1
        moved = True
        out["hist_x"].append(x.copy()); out["hist_f"].append(f); out["hist_k"].append(k)


def train_optimize(fun, design, Nopts, Ncov, Nnoise, LB, UB, TolFun, MaxIter=1000, MaxFunEvals=3000, fill=True, margin=None):
    """gplite_train.m:200-306 over ``design`` (rows: hyp0 first, then the space-filling design).  ``fun(x) -> (f, g)``; an
    exception or a non-finite matrix is the caller's to map to NaN.  fill = False: the branch of :249-256."""
    LB, UB = np.asarray(LB, dtype=np.float64), np.asarray(UB, dtype=np.float64)
    design = np.asarray(design, dtype=np.float64)
    fvals = np.array([fun(r)[0] for r in design])
    if fill:
        fs, order, starts, widths = select_starts(design, fvals, Nopts, Ncov, Nnoise, LB, UB)
    else:
        fs, order = matlab_sort(fvals)
        starts = np.array([clamp_in(h, LB, UB) for h in design[order][:Nopts]])
        starts[:, LB == UB] = LB[LB == UB]
        widths, order = None, order.astype(np.int32)
    runs = [pbfgs(fun, s0, LB, UB, TolFun, MaxIter, MaxFunEvals, margin) for s0 in starts]
    nll = np.array([r["f"] for r in runs])
    best = 0 if np.all(np.isnan(nll)) else int(np.nanargmin(nll))
    hyp_start = clamp_in(runs[best]["x"], LB, UB)
    hyp_start[LB == UB] = LB[LB == UB]
    return dict(fill_fvals=fs, fill_order=order, widths_default=widths, starts=starts, runs=runs, hyp=np.array([r["x"] for r in runs]).T,
                nll=nll, best=best, hyp_start=hyp_start)

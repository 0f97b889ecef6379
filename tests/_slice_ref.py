"""NumPy restatement of the reference's bounded slice sampler, one evaluation at a time (test infrastructure).

``slicesamplebnd(logf, x0, N, widths, LB, UB, options, perms, U)`` restates utils/slicesamplebnd.m:157-205 (start-up) and :229-358 (the
main loop) with StepOut = false and no LogPrior option, and its local logpdfbound (:415-449).  The random numbers come from an INDEXED
block instead of a stream, so that a speculative implementation can be fed the same draws:

  perms[sweep]            0-based permutation of the coordinates (randperm(D) - 1, :239)
  U[sweep, idd, 0]        the slice level's rand (:245)
  U[sweep, idd, 1]        the interval placement's rand (:252)
  U[sweep, idd, 2 + k]    the k-th shrink proposal's rand, k = 0, 1, ... (:286)

MATLAB's max / min pass over a NaN operand (np.fmax / np.fmin); eps(x) is np.spacing(abs(x)), NaN for an infinite x.
"""
import numpy as np


class SliceCollapse(RuntimeError):
    pass


def matlab_eps(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.spacing(x), np.nan)


def make_block(rng, sweeps, D, Kmax):
    perms = np.stack([rng.permutation(D) for _ in range(sweeps)]).astype(np.int32)
    U = rng.random((sweeps, D, 2 + Kmax))
    return perms, U


def slicesamplebnd(logf, x0, N, widths, LB, UB, options, perms, U):
    """Returns samples (N x D), fvals (N), output dict {widths, funccount, maxshrink}."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    D = x0.size
    LB = np.broadcast_to(np.asarray(-np.inf if LB is None else LB, dtype=np.float64), (D,)).copy()
    UB = np.broadcast_to(np.asarray(np.inf if UB is None else UB, dtype=np.float64), (D,)).copy()
    thin = int(np.floor(options.get("Thin", 1)))
    burn = int(np.floor(options.get("Burnin", round(N / 3))))
    adaptive = bool(options.get("Adaptive", True))
    LB_out = LB - matlab_eps(LB)                                             # :164-165
    UB_out = UB + matlab_eps(UB)
    basewidths = None if widths is None else np.broadcast_to(np.asarray(widths, dtype=np.float64), (D,)).copy()   # :166
    if widths is None:
        widths = (UB - LB) / 2                                               # :173
    widths = np.broadcast_to(np.asarray(widths, dtype=np.float64), (D,)).copy()
    widths[np.isinf(widths)] = 10                                            # :174
    count = {"n": 0}

    def logpdfbound(x):                                                      # :415-449
        if np.any((x < LB) | (x > UB)):
            return -np.inf
        fval = logf(x)
        count["n"] += 1
        return -np.inf if np.isnan(fval) else float(fval)

    y = logpdfbound(x0)                                                      # :177
    xx = x0.copy()
    samples = np.zeros((N, D))
    fvals = np.zeros(N)
    log_Px = y
    widths[LB == UB] = 1                                                     # :185
    assert np.all(UB >= LB) and np.all((widths > 0) & np.isfinite(widths))
    assert np.all(x0 >= LB) and np.all(x0 <= UB) and np.isfinite(y) and thin > 0 and burn >= 0
    effN = N + (N - 1) * (thin - 1)                                          # :205
    xx_sum = np.zeros(D)
    xx_sqsum = np.zeros(D)
    maxshrink = 0
    for ii in range(1, effN + burn + 1):                                     # :229
        dvec = perms[ii - 1]
        for idd in range(D):
            dd = int(dvec[idd])
            if LB[dd] == UB[dd]:
                continue                                                     # :243
            u = U[ii - 1, idd]
            log_uprime = np.log(u[0]) + log_Px                               # :245
            x_l = xx.copy()
            x_r = xx.copy()
            xprime = xx.copy()
            rr = u[1]
            x_l[dd] = xx[dd] - rr * widths[dd]                               # :253-254
            x_r[dd] = xx[dd] + (1 - rr) * widths[dd]
            if np.isfinite(LB[dd]) or np.isfinite(UB[dd]):                   # :257-260
                x_l[dd] = np.fmax(x_l[dd], LB_out[dd])
                x_r[dd] = np.fmin(x_r[dd], UB_out[dd])
            shrink = 0
            while True:                                                      # :283-304
                if 2 + shrink >= u.size:
                    raise IndexError("uniform block exhausted (Kmax = %d)" % (u.size - 2))
                xprime[dd] = u[2 + shrink] * (x_r[dd] - x_l[dd]) + x_l[dd]
                shrink += 1
                log_Px = logpdfbound(xprime)
                if log_Px > log_uprime:
                    break
                if xprime[dd] > xx[dd]:
                    x_r[dd] = xprime[dd]
                elif xprime[dd] < xx[dd]:
                    x_l[dd] = xprime[dd]
                else:
                    raise SliceCollapse("Shrunk to current position and proposal still not acceptable.")
            maxshrink = max(maxshrink, shrink)
            if ii <= burn and adaptive:                                      # :307-318
                delta = UB[dd] - LB[dd]
                if shrink > 3:
                    widths[dd] = np.fmax(widths[dd] / 1.1, np.spacing(delta) if np.isfinite(delta) else np.finfo(np.float64).eps)
                elif shrink < 2:
                    widths[dd] = np.fmin(widths[dd] * 1.2, delta)
            xx[dd] = xprime[dd]                                              # :325
        if ii > burn and (ii - burn - 1) % thin == 0:                        # :331-337
            ismpl = (ii - burn - 1) // thin
            samples[ismpl] = xx
            fvals[ismpl] = log_Px
        if ii <= burn and ii > burn / 2:                                     # :340-358
            xx_sum = xx_sum + xx
            xx_sqsum = xx_sqsum + xx * xx
            if ii == burn and adaptive:
                burnstored = burn // 2
                with np.errstate(invalid="ignore", divide="ignore"):
                    var = xx_sqsum / burnstored - (xx_sum / burnstored) ** 2
                    newwidths = np.fmin(5 * np.sqrt(var), UB_out - LB_out)
                if np.any(var < 0):                                          # ~isreal(newwidths)
                    newwidths = widths.copy()
                widths = newwidths if basewidths is None else np.fmax(newwidths, np.sqrt(newwidths * basewidths))
    return samples, fvals, {"widths": widths, "funccount": count["n"], "maxshrink": maxshrink}

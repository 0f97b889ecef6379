"""Restatement of the multi-run diagnostics for the tests: the decision of vbmc_diagnostics.m:58-114, :129-222 as plain loops over the
runs, written from its logic (exit flags, not messages), the NaN-skipping maximum of :124, the argument defaults as the reference's
:53-56 actually behave, and the runs of the GPU cases.  Host NumPy only."""
import math

import numpy as np


def first_max(v):
    """[~, idx] = max(v) of MATLAB, from 0: the first largest entry among those that are not NaN; 0 if all are NaN"""
    idx, top = 0, None
    for i, x in enumerate(v):
        if x != x:
            continue
        if top is None or x > top:
            idx, top = i, x
    return idx


def nanskip_max(row):
    """max(row) of MATLAB: NaN entries are skipped; NaN if all are"""
    top = math.nan
    for x in row:
        if x == x and not (top >= x):
            top = x
    return top


def decision(elbo, elbo_sd, stable, kl_mat, maxmtv_mat, beta_lcb=3, elbo_thresh=1, sKL_thresh=1, maxmtv_thresh=0.2):
    n = len(elbo)
    flag = math.inf
    nconv = sum(1 for s in stable if s)
    active = [bool(s) for s in stable]
    if nconv == 0:
        active = [True] * n
        flag = -3
    elif nconv == 1:
        flag = 0
    elcbo = [elbo[i] - beta_lcb * elbo_sd[i] for i in range(n)]
    best = first_max([elcbo[i] if active[i] else -math.inf for i in range(n)])
    skl = [0.5 * (kl_mat[i][best] + kl_mat[best][i]) for i in range(n)]
    mm = [maxmtv_mat[best][i] for i in range(n)]
    if n > 1:
        need = max(n * (1 / 3), 2)
        if sum(1 for i in range(n) if abs(elbo[best] - elbo[i]) < elbo_thresh) < need:
            flag = min(flag, -2)
        if sum(1 for i in range(n) if skl[i] < sKL_thresh) < need:
            flag = min(flag, -1)
        if sum(1 for i in range(n) if mm[i] < maxmtv_thresh) < need:
            flag = min(flag, -1)
    if math.isinf(flag):
        flag = 1
    return dict(exitflag=int(flag), best_run=best, idx_best=best if stable[best] else None, elcbo=np.array(elcbo), sKL_best=np.array(skl),
                maxmtv_best=np.array(mm))


def reference_arguments(*given):
    """(beta_lcb, elbo_thresh, sKL_thresh, maxmtv_thresh) as vbmc_diagnostics.m:53-56 leave them when a caller gives `given` after
    vp_array: the tests compare nargin (1 + len(given)) with a number one too high, so the LAST argument given is replaced by its
    default.  (The help text, :30-49, says a given argument is used: that is what the library does.)"""
    nargin = 1 + len(given)
    vals = list(given) + [None] * (4 - len(given))
    out = []
    for pos, default in enumerate((3, 1, 1, 0.2)):
        out.append(default if nargin < 3 + pos or vals[pos] is None else vals[pos])
    return tuple(out)


def with_stats(vp, elbo, elbo_sd=0.01, stable=True):
    out = dict(vp)
    out["stats"] = dict(elbo=elbo, elbo_sd=elbo_sd, stable=stable)
    return out


def runs(case, R, width=1.0):
    """make_case(case) and R - 1 siblings of it, sibling i with seed 2 + i"""
    from tests import _vptools_ref as T

    vp = T.make_case(case, width=width)
    return [vp] + [T.sibling(vp, seed=2 + i) for i in range(R - 1)]

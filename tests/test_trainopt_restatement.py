"""CPU checks of the optimisation half of gplite_train: the NumPy restatement of the library's projected-BFGS optimiser
(tests/_trainopt_ref.py) against closed forms and scipy's L-BFGS-B, the design map of fminfill (vbmc_amd.fminfill_design), the
fill stage's bookkeeping, the ABI plumbing of vbmc_gp_train_optimize and a cross-compile of its kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import minimize

from tests import _abi
from tests import _trainopt_ref as T
from tests._trainopt_cases import PARITY_CASES, WIDE_CASES, gp_case, parity_case, parity_sizes

ROOT, CSRC = _abi.ROOT, _abi.CSRC


# ---- the optimiser ----------------------------------------------------------------------------------------------------------
def _quad(seed, n):
    """A convex quadratic whose box cuts off its free minimiser: the bounded minimiser comes from scipy's bounded least squares."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((2 * n, n))
    Q = A.T @ A / n + 0.5 * np.eye(n)
    xs = rng.standard_normal(n) * 2.0
    b = Q @ xs
    LB, UB = np.full(n, -1.0), np.full(n, 1.0)
    LB[0] = -np.inf
    return Q, b, LB, UB


@pytest.mark.parametrize("seed,n", [(0, 4), (1, 7), (2, 12)])
def test_bounded_quadratic_reaches_the_kkt_point(seed, n):
    Q, b, LB, UB = _quad(seed, n)
    fun = lambda x: (0.5 * x @ Q @ x - b @ x, Q @ x - b)
    # TolFun far below the bounds asserted: the |df| <= TolFun (1 + |f|) rule may stop the run a modest multiple of TolFun above the
    # minimum.  Q >= I / 2, so f - f* <= 1e-9 (1 + |f*|) (about 1e-8 here) bounds |x - x*|^2 by 2 (f - f*) / (1 / 2) = 4e-8.
    tol = 1e-12
    r = T.pbfgs(fun, np.zeros(n), LB, UB, tol, MaxIter=500)
    ref = minimize(lambda x: fun(x), np.zeros(n), jac=True, method="L-BFGS-B", bounds=list(zip(LB, UB)), options={"ftol": 1e-15, "gtol": 1e-12})
    x = r["x"]
    assert np.sum((x == LB) | (x == UB)) >= 1                      # the bounds are active at the optimum
    assert r["exitflag"] in (T.EXIT_GRAD, T.EXIT_DF), r["exitflag"]
    assert r["f"] - ref.fun <= 1e-9 * (1 + abs(ref.fun)), (r["f"], ref.fun)
    assert np.max(np.abs(x - ref.x)) <= 2e-4 + 1e-5                # (1e-5: scipy's own distance from the minimiser)


def test_bounded_rosenbrock():
    def fun(x):
        f = 100.0 * (x[1] - x[0] ** 2) ** 2 + (1 - x[0]) ** 2
        return f, np.array([-400.0 * x[0] * (x[1] - x[0] ** 2) - 2 * (1 - x[0]), 200.0 * (x[1] - x[0] ** 2)])
    # free: the minimiser (1, 1)
    r = T.pbfgs(fun, np.array([-1.2, 1.0]), np.array([-2.0, -2.0]), np.array([2.0, 2.0]), 1e-10, MaxIter=2000, MaxFunEvals=10000)
    assert np.max(np.abs(r["x"] - 1.0)) < 1e-4, r
    # x0 <= 0.5: the minimiser is (0.5, 0.25), on the bound
    r = T.pbfgs(fun, np.array([-1.2, 1.0]), np.array([-2.0, -2.0]), np.array([0.5, 2.0]), 1e-10, MaxIter=2000, MaxFunEvals=10000)
    assert r["x"][0] == 0.5 and abs(r["x"][1] - 0.25) < 1e-4, r


def test_fixed_coordinates_never_move_and_nan_is_a_rejection():
    calls = []
    def fun(x):
        calls.append(x.copy())
        if x[0] > 0.8:
            return np.nan, np.full(3, np.nan)
        return np.sum((x - 2.0) ** 2), 2.0 * (x - 2.0)
    LB, UB = np.array([-5.0, 0.3, -5.0]), np.array([5.0, 0.3, 5.0])
    r = T.pbfgs(fun, np.array([0.0, 0.3, 0.0]), LB, UB, 1e-9)
    assert all(c[1] == 0.3 for c in calls) and r["x"][1] == 0.3
    assert r["funccount"] == len(calls) and np.isfinite(r["f"]) and r["x"][0] <= 0.8
    r = T.pbfgs(lambda x: (np.nan, np.zeros(3)), np.zeros(3), LB, UB, 1e-9)
    assert r["exitflag"] == T.EXIT_START and r["funccount"] == 1


ORACLE_GAP_MARGIN = 1e-3


@pytest.mark.parametrize("meanfun,noisefun,prior", [(4, (1, 0, 0), "student"), (1, (1, 1, 0), "gauss")])
def test_oracle_objective_not_worse_than_lbfgsb(meanfun, noisefun, prior):
    """gplite_nlZ of the oracle with a hyper-prior on two small GPs, TolFun 1e-6 against scipy's L-BFGS-B (ftol 1e-12) from the same start.
    Measured on the CPU when the test was written: f_pbfgs - f_scipy = +1.993e-06 (meanfun 4, Student-t; 53 iterations, 67
    evaluations, stopped by the |df| rule) and +1.923e-09 (meanfun 1, Gaussian; 23 iterations, 25 evaluations); the bound is that
    gap plus a margin, 1e-3 in all: a thousandth of a nat of log marginal likelihood."""
    from oracle import vbmc_ref as R

    c = gp_case(5, D=2, N=25, meanfun=meanfun, noisefun=noisefun, prior=prior)
    def fun(h):
        try:
            f, g = R.gplite_nlZ(h, c["gp"], c["hprior"], True)
            return float(f), np.asarray(g, dtype=np.float64).reshape(-1)
        except Exception:
            return np.nan, np.full(h.size, np.nan)
    x0 = T.clamp_in(c["h0"], c["LB"], c["UB"])
    r = T.pbfgs(fun, x0, c["LB"], c["UB"], 1e-6)
    ref = minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(c["LB"], c["UB"])), options={"maxiter": 1000, "ftol": 1e-12, "gtol": 1e-8})
    print("oracle objective: pbfgs %.12g (it %d, fc %d, flag %d)  scipy %.12g  gap %.3e" % (r["f"], r["iterations"], r["funccount"], r["exitflag"],
                                                                                          ref.fun, r["f"] - ref.fun))
    assert r["f"] - ref.fun <= ORACLE_GAP_MARGIN, (r["f"], ref.fun)


@pytest.mark.parametrize("ci", range(len(PARITY_CASES)))
def test_parity_cases_are_decidable_and_well_conditioned(ci):
    """The two conditions under which the GPU parity cases were chosen (tests/_trainopt_cases.py), with the oracle's objective:
    every Armijo / stopping decision and every gap between fill values at least 1e-6 relative from flipping, and iterates that a
    1e-13 relative perturbation of the gradient (two draws) moves by at most 1e-10.  The wide cases (8 on) also meet the third, that
    the oracle's value at every iterate is settled to 1e-11, and those with Nhyp > 64 reach the full H product."""
    import vbmc_amd as va
    from oracle import vbmc_ref as R

    c, tol, maxit = parity_case(ci)

    def make(eps, seed):
        rng = np.random.default_rng(seed)

        def fun(h):
            try:
                f, g = R.gplite_nlZ(h, c["gp"], c["hprior"], True)
            except Exception:
                return np.nan, np.full(h.size, np.nan)
            f, g = float(f), np.asarray(g, dtype=np.float64).reshape(-1)
            if not np.isfinite(f):
                return np.nan, np.full(h.size, np.nan)
            return f, g * (1.0 + eps * rng.standard_normal(g.size))
        return fun

    Ninit, Nopts = parity_sizes(ci)
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], Ninit, seed=3)
    run = lambda fun, m=None: T.train_optimize(fun, design, Nopts, c["gp"]["Ncov"], c["gp"]["Nnoise"], c["LB"], c["UB"], tol, MaxIter=maxit, margin=m)
    margin = []
    base = run(make(0.0, 0), margin)
    fin = base["fill_fvals"][np.isfinite(base["fill_fvals"])]
    assert min(margin) > 1e-6 and np.min(np.diff(fin)) > 1e-6, (min(margin), np.min(np.diff(fin)))
    worst = 0.0
    for seed in (1, 2):
        pert = run(make(1e-13, seed))
        for r0, r1 in zip(base["runs"], pert["runs"]):
            assert r0["iterations"] == r1["iterations"] and r0["hist_k"] == r1["hist_k"] and r0["exitflag"] == r1["exitflag"]
            if r0["iterations"]:
                a, b = np.array(r1["hist_x"]), np.array(r0["hist_x"])
                worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))))
    print("case %d: margin %.2e, moved %.2e, %r" % (ci, min(margin), worst, [(r["iterations"], r["exitflag"]) for r in base["runs"]]))
    assert worst <= 1e-10, worst
    if ci in WIDE_CASES:
        # condition 3: the oracle's own value at every iterate is settled far below the 1e-10 it is the yardstick for
        X, pts = c["gp"]["X"], [x for r in base["runs"] for x in r["hist_x"]]
        val = lambda gp: np.array([float(R.gplite_nlZ(x, gp, c["hprior"], False)[0]) for x in pts])
        v0, settled = val(c["gp"]), 0.0
        for seed in (1, 2):
            v1 = val(dict(c["gp"], X=X * (1.0 + 2.0 ** -52 * np.random.default_rng(seed).standard_normal(X.shape))))
            settled = max(settled, float(np.max(np.abs(v1 - v0) / np.maximum(1.0, np.abs(v0)))))
        print("case %d: one unit in the last place of X moves the oracle's values by %.2e" % (ci, settled))
        assert settled <= 1e-11, settled
    if c["h0"].size > 64:
        # the cases that are there for the H products beyond lane 63 reach them: every start moves at least three times, and from the
        # third step on the step is not along the gradient (a step with the identity in H's place is, exactly: cosine 1; the cosines
        # here were at most 0.99972 when the cases were chosen)
        exact = make(0.0, 0)
        for r in base["runs"]:
            assert r["iterations"] >= 3
            hx = np.array(r["hist_x"])
            for k in range(2, r["iterations"]):
                m = np.all((hx[k - 1:k + 1] > c["LB"]) & (hx[k - 1:k + 1] < c["UB"]), axis=0)    # (the coordinates no bound cuts short)
                s, g = (hx[k] - hx[k - 1])[m], exact(hx[k - 1])[1][m]
                assert np.sum(m) >= 60 and -(s @ g) < (1.0 - 1e-6) * np.linalg.norm(s) * np.linalg.norm(g), (k, np.sum(m), s @ g)


# ---- the design map ---------------------------------------------------------------------------------------------------------
def test_uuinv_break_points_and_degenerate_branches():
    import vbmc_amd as va

    nv = 3
    w = 0.5 ** (1.0 / nv)
    LB, PLB, PUB, UB = np.array([-4.0, 0.0, -np.inf]), np.array([-1.0, 0.0, -1.0]), np.array([2.0, 0.0, 1.0]), np.array([6.0, 0.0, np.inf])
    L = (6.0 - (-4.0)) + (-1.0) - 2.0
    t1 = (1 - w) * (PLB[0] - LB[0]) / L
    S = np.zeros((6, nv))
    S[:, 0] = [0.0, t1, t1 + w, 1.0, 0.5 * t1, t1 + 0.5 * w]
    S[:, 1] = [0.0, 0.05, 0.5, 1.0, 0.3, 0.9]
    S[:, 2] = [0.0, 0.25, 0.5, 1.0, 0.75, 0.1]
    X = va.fminfill_design(np.zeros((1, nv)), LB, UB, PLB, PUB, None, 7, S)
    assert X.shape == (7, nv) and np.all(X[0] == 0.0)
    np.testing.assert_allclose(X[1:, 0], [-4.0, -1.0, 2.0, 6.0, -2.5, 0.5], rtol=0, atol=1e-12)
    assert np.all(X[1:, 1] == 0.0)                                          # L == 0: deltas and a zero-width uniform
    np.testing.assert_allclose(X[1:, 2], S[:, 2] * 2.0 - 1.0, rtol=0, atol=0)   # infinite bound: the plausible box alone
    # the L == 0 branch with a plausible box of positive width
    Y = va.fminfill_design(np.zeros((1, 1)), [0.0], [1.0], [0.0], [1.0], None, 4, np.array([[0.1], [0.4], [0.95]]))
    np.testing.assert_allclose(Y[1:, 0], [0.0, 0.3, 1.0], atol=1e-15)          # nvars = 1: w = 0.5: B1 | (p - 0.25) / 0.5 | B4


def test_student_t_quantile_matches_scipy_stats():
    from scipy import stats

    import vbmc_amd as va

    S = np.random.default_rng(0).random((200, 3))
    hp = {"mu": [0.5, -1.0, 2.0], "sigma": [2.0, 0.5, 1.0], "df": [7.0, 1.0, 0.0]}
    LB, UB = np.array([-3.0, -np.inf, 0.0]), np.array([4.0, np.inf, 5.0])
    X = va.fminfill_design(np.zeros((1, 3)), LB, UB, None, None, hp, 201, S)[1:]
    for i, (dist, df) in enumerate([(stats.t, 3.0), (stats.t, 1.0), (stats.norm, None)]):      # df capped at 3; df = 0: normal
        a = (df,) if df is not None else ()
        lo, hi = dist.cdf((LB[i] - hp["mu"][i]) / hp["sigma"][i], *a), dist.cdf((UB[i] - hp["mu"][i]) / hp["sigma"][i], *a)
        ref = dist.ppf(lo + (hi - lo) * S[:, i], *a) * hp["sigma"][i] + hp["mu"][i]
        np.testing.assert_allclose(X[:, i], ref, rtol=1e-10, atol=1e-10)
        assert np.all(X[:, i] >= LB[i]) and np.all(X[:, i] <= UB[i])


# ---- fill-stage bookkeeping -------------------------------------------------------------------------------------------------
def test_sort_starts_low_noise_pick_and_widths():
    f = np.array([3.0, np.nan, 1.0, 3.0, -np.inf, np.nan, 1.0, 2.0])
    fs, order = T.matlab_sort(f)
    assert list(order) == [4, 2, 6, 7, 0, 3, 1, 5] and np.isnan(fs[-2:]).all()
    # design: Ncov = 1, one noise parameter in column 1, column 2 constant (zero width), column 3 constant over the starts only
    design = np.array([[0.0, 5.0, 7.0, 1.0], [1.0, 4.0, 7.0, 2.0], [2.0, -3.0, 7.0, 4.0], [3.0, 2.0, 7.0, 3.0], [4.0, 1.0, 7.0, 4.0],
                       [5.0, -2.0, 7.0, 5.0], [6.0, -1.0, 7.0, 4.0], [7.0, 0.0, 7.0, 6.0]])
    LB, UB = np.array([-10.0, -10.0, 6.5, -np.inf]), np.array([10.0, 10.0, 7.25, np.inf])
    fs, order, starts, widths = T.select_starts(design, f, 2, 1, 1, LB, UB)
    # sorted rows: 4 2 6 7 0 3 1 5; the rest after two starts: 6 7 0 3 1 5 with noise -1 0 5 2 4 -2 -> by noise: 5 6 7 3 1 0;
    # ceil(0.2 * 6) = 2 of them: rows 5 (NaN) and 6 (1.0) -> row 6
    assert np.all(starts[0] == design[4]) and np.all(starts[1] == design[6])
    assert widths[2] == 0.75 and np.all(widths[[0, 1, 3]] > 0)                 # std 0, std over the starts 0 -> min(1, UB - LB)
    np.testing.assert_allclose(widths[0], np.std(design[:, 0], ddof=1))
    # the clamp: an infinite bound leaves the coordinate alone, a start on a bound moves inside by eps
    st = T.clamp_in(np.array([-10.0, 10.0, 7.0, 1e300]), LB, UB)
    assert st[0] == -10.0 + np.spacing(10.0) and st[1] == 10.0 - np.spacing(10.0) and st[3] == 1e300


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_library_and_ctypes():
    from vbmc_amd import _lib

    hdr = _abi.header_text()
    assert re.search(r"vbmc_status\s+vbmc_gp_train_optimize\s*\(\s*vbmc_ctx\s*\*\s*ctx\s*,\s*const\s+vbmc_gptrain_args\s*\*", hdr)
    assert int(re.search(r"#define\s+VBMC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.vbmc_gp_train_optimize.argtypes[1]._type_ is _lib.GpTrainArgs
    # (the mirror's layout against the header's: tests/test_abi_symbols.py)
    # struct_size is checked before anything else is read (no device needed: a null context is refused first, a wrong size next)
    a = _lib.new_args(_lib.GpTrainArgs)
    a.struct_size -= 8
    assert lib.vbmc_gp_train_optimize(None, C.byref(a)) == _lib.VBMC_ERR_INVALID
    src = open(os.path.join(CSRC, "abi_gp_train.hip")).read()
    assert "args->struct_size != sizeof(vbmc_gptrain_args)" in src


def test_trainopt_kernels_compile_for_gfx950_without_scratch(tmp_path):
    kernels, _ = _abi.kernel_meta("trainopt_kernels.h", (), r"k_(topt|gpobj)_", tmp_path, flags=("-Wno-pass-failed",))
    seen = set()
    for k in kernels:
        assert _abi.no_scratch(k), k
        seen.add(k["name"])
    assert seen == {"k_topt_propose", "k_gpobj_retry", "k_topt_fill_collect", "k_topt_fill_sort", "k_topt_decide", "k_topt_close"}, seen

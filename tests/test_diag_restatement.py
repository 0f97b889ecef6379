"""CPU: the decision part of vbmc_diagnostics (vbmc_amd.vptools.diagnostics_decision, a pure host function of the runs' statistics and
the two distance matrices) on hand-made matrices, against the expected exit flags and against the loop restatement tests/_diag_ref.py:
every exit flag (1, 0, -1 through the KL divergence alone, -1 through the total variation alone, -2, -3), the agreement threshold
max(Nruns / 3, 2) at Nruns = 2, 3, 6 and 7, NaN in the ELCBO and in a row of maxmtv_mat, a best run that is not stable, one run (no
device call), and the two quirks of the reference: its argument defaults overwrite the last argument given (the library uses it), and
the maximum over the dimensions skips NaN."""
import inspect
import math
import warnings

import numpy as np
import pytest

from tests import _diag_ref as R


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import vptools

    return vptools


def mats(n, kl=0.1, mm=0.05):
    k = np.full((n, n), float(kl))
    m = np.full((n, n), float(mm))
    np.fill_diagonal(k, 0.0)
    np.fill_diagonal(m, 0.0)
    return k, m


def both(V, elbo, sd, stable, kl, mm, *thr):
    got = V.diagnostics_decision(elbo, sd, stable, kl, mm, *thr)
    want = R.decision(list(elbo), list(sd), list(stable), np.asarray(kl).tolist(), np.asarray(mm).tolist(), *thr)
    assert got["exitflag"] == want["exitflag"] and got["idx_best"] == want["idx_best"] and got["best_run"] == want["best_run"], (got, want)
    for k in ("elcbo", "sKL_best", "maxmtv_best"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    return got


def test_every_exit_flag(V):
    n = 3
    elbo, sd, ok = np.array([-1.0, -1.2, -0.9]), np.full(n, 0.05), np.ones(n, bool)
    kl, mm = mats(n)
    g = both(V, elbo, sd, ok, kl, mm)
    assert g["exitflag"] == 1 and g["idx_best"] == 2 and g["msg"].endswith("PASSED.")
    assert both(V, elbo, sd, [False, True, False], kl, mm)["exitflag"] == 0                  # one converged run, everything agrees
    far = kl.copy()
    far[2, :2] = far[:2, 2] = 5.0
    g = both(V, elbo, sd, ok, far, mm)                                                        # the KL divergence alone
    assert g["exitflag"] == -1 and np.sum(g["sKL_ok"]) == 1 and np.all(g["maxmtv_ok"]) and np.all(g["elbo_ok"])
    wide = mm.copy()
    wide[2, :2] = wide[:2, 2] = 0.5
    g = both(V, elbo, sd, ok, kl, wide)                                                       # the total variation alone
    assert g["exitflag"] == -1 and np.all(g["sKL_ok"]) and np.sum(g["maxmtv_ok"]) == 1 and np.all(g["elbo_ok"])
    g = both(V, np.array([-11.0, -12.0, -0.9]), sd, ok, kl, mm)                               # the ELBO alone
    assert g["exitflag"] == -2 and np.all(g["sKL_ok"]) and np.all(g["maxmtv_ok"])
    assert both(V, np.array([-11.0, -12.0, -0.9]), sd, ok, far, wide)["exitflag"] == -2      # min(exitflag, .): -2 wins over -1
    g = both(V, elbo, sd, np.zeros(n, bool), kl, mm)                                          # nothing converged: all runs compete
    assert g["exitflag"] == -3 and g["best_run"] == 2 and g["idx_best"] is None
    assert both(V, elbo, sd, np.zeros(n, bool), far, mm)["exitflag"] == -3                    # -3 stays below -1
    far1 = kl.copy()
    far1[1, [0, 2]] = far1[[0, 2], 1] = 5.0
    assert both(V, elbo, sd, [False, True, False], far1, mm)["exitflag"] == -1                # 0 does not survive a failed check


def test_elcbo_picks_the_first_maximum_among_converged_runs(V):
    kl, mm = mats(4)
    elbo, sd = np.array([0.0, 0.0, -0.5, 5.0]), np.array([0.1, 0.1, 0.0, 0.1])
    g = both(V, elbo, sd, [True, True, True, False], kl, mm, 3, 10)                           # run 3 is the largest but has not converged
    assert g["best_run"] == 0 and np.allclose(g["elcbo"], [-0.3, -0.3, -0.5, 4.7])            # runs 0 and 1 tie: the first
    assert both(V, elbo, sd, [True, True, True, False], kl, mm, 10, 10)["best_run"] == 2      # beta_lcb = 10 prefers the run without error
    asym = kl.copy()
    asym[0, 2], asym[2, 0] = 0.5, 1.0
    g = both(V, elbo, sd, [True] * 4, asym, mm, 3, 10)
    assert g["best_run"] == 3 and g["sKL_best"][3] == 0.0
    assert both(V, elbo, sd, [True, True, True, False], asym, mm, 3, 10)["sKL_best"][2] == 0.75


@pytest.mark.parametrize("n,need", [(2, 2), (3, 2), (6, 2), (7, 3)])
def test_agreement_threshold(V, n, need):
    """sum(ok) < max(Nruns / 3, 2): the best run and need - 1 others pass, one fewer fails; for each of the three checks"""
    elbo0, sd, ok = np.zeros(n), np.full(n, 0.01), np.ones(n, bool)
    elbo0[0] = 0.5                                                                            # run 0 is the best
    for agreeing, flagged in ((need, False), (need - 1, True)):
        off = np.arange(n) >= agreeing                                                        # the runs that disagree with run 0
        kl, mm = mats(n)
        kl[0, off] = kl[off, 0] = 9.0
        assert both(V, elbo0, sd, ok, kl, mats(n)[1])["exitflag"] == (-1 if flagged else 1), (n, agreeing, "sKL")
        mm[0, off] = mm[off, 0] = 0.9
        assert both(V, elbo0, sd, ok, mats(n)[0], mm)["exitflag"] == (-1 if flagged else 1), (n, agreeing, "mtv")
        elbo = elbo0.copy()
        elbo[off] = -20.0
        assert both(V, elbo, sd, ok, *mats(n))["exitflag"] == (-2 if flagged else 1), (n, agreeing, "elbo")
    assert math.ceil(max(n / 3, 2)) == need


def test_the_given_last_argument_is_used(V):
    """Quirk 1: vbmc_diagnostics.m:53-56 overwrite the last argument a caller gives; the library follows the help text"""
    assert R.reference_arguments() == (3, 1, 1, 0.2)
    assert R.reference_arguments(5) == (3, 1, 1, 0.2)                    # beta_lcb = 5 is lost
    assert R.reference_arguments(5, 2) == (5, 1, 1, 0.2)
    assert R.reference_arguments(5, 2, 4) == (5, 2, 1, 0.2)
    assert R.reference_arguments(5, 2, 4, 0.5) == (5, 2, 4, 0.2)         # and so is maxmtv_thresh = 0.5
    n = 3
    elbo, sd, ok = np.zeros(n), np.full(n, 0.01), np.ones(n, bool)
    kl, mm = mats(n, mm=0.3)
    assert both(V, elbo, sd, ok, kl, mm, 3, 1, 1, 0.5)["exitflag"] == 1                      # the library: 0.3 < 0.5
    assert both(V, elbo, sd, ok, kl, mm, *R.reference_arguments(3, 1, 1, 0.5))["exitflag"] == -1   # the reference: 0.3 > 0.2
    kl5, _ = mats(n, kl=3.0)
    assert both(V, elbo, sd, ok, kl5, mats(n)[1], 3, 1, 4)["exitflag"] == 1
    assert both(V, elbo, sd, ok, kl5, mats(n)[1], *R.reference_arguments(3, 1, 4))["exitflag"] == -1
    sig = inspect.signature(V.vbmc_diagnostics)
    names = list(sig.parameters)
    assert names[:5] == ["vp_array", "beta_lcb", "elbo_thresh", "sKL_thresh", "maxmtv_thresh"]
    assert [sig.parameters[k].default for k in names[1:5]] == [3, 1, 1, 0.2]
    assert [k for k in names[5:]] == ["Ns", "seed", "nkde", "nquad", "stages", "verbose", "engine"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[5:])
    doc = V.vbmc_diagnostics.__doc__
    assert "nargin" in doc and ":53-56" in doc and "skips NaN" in doc and ":124" in doc


def test_nan_is_skipped_by_max(V):
    """Quirk 2 (vbmc_diagnostics.m:124) and MATLAB's [~, idx] = max(.) at :114"""
    nan = math.nan
    assert R.nanskip_max([0.1, nan, 0.3]) == 0.3 and R.nanskip_max([nan, 0.2]) == 0.2 and math.isnan(R.nanskip_max([nan, nan]))
    assert R.first_max([nan, 1.0, 1.0]) == 1 and R.first_max([nan, nan]) == 0 and R.first_max([-math.inf, nan]) == 0
    kl, mm = mats(3)
    elbo, ok = np.array([0.0, 0.1, 0.2]), np.ones(3, bool)
    g = both(V, elbo, np.array([0.01, 0.01, nan]), ok, kl, mm)                                # a NaN ELCBO never is the best
    assert g["best_run"] == 1 and math.isnan(g["elcbo"][2]) and g["exitflag"] == 1
    g = both(V, np.array([0.0, 0.1, nan]), np.full(3, 0.01), ok, kl, mm)                      # and a NaN ELBO agrees with nothing
    assert g["best_run"] == 1 and list(g["elbo_ok"]) == [True, True, False] and g["exitflag"] == 1
    g = both(V, np.full(3, nan), np.full(3, 0.01), ok, kl, mm)                                # all NaN: the first run, no agreement
    assert g["best_run"] == 0 and g["exitflag"] == -2
    hole = mm.copy()
    hole[1, 2] = hole[2, 1] = nan
    g = both(V, elbo, np.array([0.01, 0.01, nan]), ok, kl, hole)                              # NaN in the best run's row: no agreement
    assert list(g["maxmtv_ok"]) == [True, True, False] and g["exitflag"] == 1
    hole[1, 0] = hole[0, 1] = nan
    assert both(V, elbo, np.array([0.01, 0.01, nan]), ok, kl, hole)["exitflag"] == -1


def test_unstable_best(V):
    kl, mm = mats(2)
    g = both(V, np.array([1.0, 0.5]), np.array([0.0, math.nan]), [False, True], kl, mm)   # eff = [-Inf, NaN]: the first, unstable
    assert g["best_run"] == 0 and g["idx_best"] is None and g["exitflag"] == 0
    g = both(V, np.array([1.0, 0.9]), np.zeros(2), [False, False], kl, mm)
    assert g["best_run"] == 0 and g["idx_best"] is None and g["exitflag"] == -3


def test_one_run_needs_no_device(V):
    from tests import _mtv_ref as M

    for stable, flag in ((True, 0), (False, -3)):
        g = both(V, [1.0], [0.1], [stable], [[0.0]], [[0.0]])
        assert g["exitflag"] == flag and g["elbo_ok"] is None
        vp = R.with_stats(M._gauss(2, 0.0, 1.0), 1.0, 0.1, stable)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            exitflag, best, idx, stats = V.vbmc_diagnostics([vp], verbose=False, engine=object())   # an engine that cannot run anything
        assert any("several runs" in str(x.message) for x in w)
        assert exitflag == flag and stats["exitflag"] == flag and np.array_equal(stats["kl_mat"], [[0.0]]) and np.array_equal(stats["maxmtv_mat"], [[0.0]])
        assert (idx, None if best is None else best["vp"] is vp) == ((0, True) if stable else (None, None))
        assert set(stats) >= {"beta_lcb", "elbo_thresh", "sKL_thresh", "maxmtv_thresh", "elbo", "elbo_sd", "elcbo", "idx_best", "sKL_best",
                              "maxmtv_best", "kl_mat", "maxmtv_mat", "exitflag", "msg"}

"""CPU: the extended-precision restatement tests/_pred_ref.py against the float64 oracle on every case of tests/_pred_cases.py, the
power condition of those cases, and the figures the device's tolerances are built from.

The float64 oracle (oracle/vbmc_ref.gplite_pred, tests/_quad_ref.gplite_quad) is the reference's own arithmetic: sq_dist's expansion
on centred inputs, BLAS sums, LAPACK substitution.  Its worst error against the restatement, in the measures of tests/_pred_ref.py and
over all cases, is E_REF_V (fs2, ys2, varF) and E_REF_M (fmu, F): what this test measured (printed with -s).  The device is held to
32 times exactly those in tests/test_gpu_pred_forms.py.  The oracle itself is locked here under CEIL_V / CEIL_M, a quarter above them,
for a BLAS that adds in another order; an oracle that stays far below the recorded figures only warns, since that too is a property of
the host's BLAS and not of the project.

What sets them is sq_dist's expansion: |a|^2 + |b|^2 - 2 a.b is rounded at ulp(|a|^2), |a|^2 is in the thousands for the low-noise
sample of a mixed GP at D >= 13 (its length scales are a quarter of the others'), and the error passes into the exponent."""
import warnings

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _pred_cases as C
from tests import _pred_ref as P
from tests import _quad_ref as Q

E_REF_V = 2880.0  # measured, in units of u (kss + vmag)
E_REF_M = 4815.0  # measured, in units of u (|m*| + sum |Ks_n alpha_n|)
CEIL_V, CEIL_M = 1.25 * E_REF_V, 1.25 * E_REF_M   # the oracle's lock
DEVICE_FACTOR = 32

_seen = {}


def oracle_errors(name):
    c, d = C.CASES[name], C.case_data(name)
    ref = d["ref"]
    if c["quad"]:
        F, V = Q.gplite_quad(d["gp"], d["Xs"], d["sigma"][None, :], True)
        return P.err_fs2(V, ref, clamp=P.EPS), P.err_fmu(F, ref), None
    _, ys2, fmu, fs2 = R.gplite_pred(d["gp"], d["Xs"], d["ys"], d["s2s"], True)
    return P.err_fs2(fs2, ref), P.err_fmu(fmu, ref), P.err_fs2(ys2, ref, field="ys2")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_agrees_with_oracle_and_case_has_power(name):
    c, d = C.CASES[name], C.case_data(name)
    assert d["Xs"].shape == (C.nstar_of(c, 256), c["D"]) and d["gp"]["X"].shape == (c["N"], c["D"]) and len(d["gp"]["post"]) == c["S"]
    pv, pm = P.assert_power(d["ref"], name)
    if c["quad"]:
        from tests.test_gpu_quad import _conditioned

        assert _conditioned(d["gp"], d["Xs"], d["sigma"]) < 1e-10
    eV, eM, eY = oracle_errors(name)
    _seen[name] = (eV, eM)
    print("%-20s Nstar %5d  power %.2f %.2f   oracle e: fs2 %8.1f  fmu %8.1f%s" % (name, d["Xs"].shape[0], pv, pm, eV, eM, "" if eY is None else "  ys2 %8.1f" % eY))
    assert eV <= CEIL_V and eM <= CEIL_M and (eY is None or eY <= CEIL_V)
    C.check_mixed(name, d["gp"])


def test_e_ref_is_what_the_oracle_reaches():
    for name in sorted(C.CASES):
        if name not in _seen:
            _seen[name] = oracle_errors(name)[:2]
    eV, eM = max(v[0] for v in _seen.values()), max(v[1] for v in _seen.values())
    print("e_ref: fs2 / ys2 / varF %.1f (E_REF_V = %g)   fmu / F %.1f (E_REF_M = %g)" % (eV, E_REF_V, eM, E_REF_M))
    assert eV <= CEIL_V and eM <= CEIL_M, "the float64 oracle is further from the restatement than recorded: %.1f, %.1f" % (eV, eM)
    if eV < E_REF_V / 2 or eM < E_REF_M / 2:
        warnings.warn("the float64 oracle reaches %.1f / %.1f here, under half the recorded e_ref %g / %g: another BLAS order, or the "
                      "recorded figures want measuring again" % (eV, eM, E_REF_V, E_REF_M))


def test_old_recipe_has_no_power_from_D13():
    """the points of tests/_cases.synth_problem's recipe (1.3 N(0, I)) in place of near_data_points: the power condition fails at D >= 13"""
    for name in ("qs_D13", "qs_D16", "qs_D20", "qs_D32", "small_D21_N20"):
        d = C.case_data(name)
        Xs = 1.3 * np.random.default_rng(5).standard_normal(d["Xs"].shape)
        pv, pm = P.power(d["gp"], Xs)
        assert pv < P.POWER_V and pm < P.POWER_M, (name, pv, pm)
    assert P.power(C.case_data("qs_D4")["gp"], 1.3 * np.random.default_rng(5).standard_normal((50, 4)))[0] > P.POWER_V


def test_near_data_points_hit_their_kernel_value():
    """k(x*, X_i) / sf2 = rho for the mean length scales: the largest cross-kernel value of a near point lies in [lo, 1] at every D"""
    for name in ("qs_D4", "qs_D20", "qs_D32"):
        gp = C.case_data(name)["gp"]
        D = gp["X"].shape[1]
        Xs = P.near_data_points(gp, 64, np.random.default_rng(3), lo=1e-2, hi=0.999)
        ell = P.mean_lengthscales(gp)
        k = np.exp(-0.5 * np.sum(((Xs[:, None, :] - gp["X"][None, :, :]) / ell) ** 2, axis=2)).max(axis=1)
        assert np.all(k >= 1e-2 * (1 - 1e-12)) and np.all(k <= 1.0), (name, D, k.min())
    gp = C.case_data("qs_D4")["gp"]
    Xs = P.near_data_points(gp, 40, np.random.default_rng(3), exact=0.25, far=0.25)
    assert sum(bool(np.any(np.all(x == gp["X"], axis=1))) for x in Xs) == 10


@pytest.mark.parametrize("shape", C.IQR_SHAPES)
def test_iqr_cases_have_power(shape):
    """the product-entry cases of the two-kernel form: test points, importance points, the cross term and the `ok` mask"""
    D = shape[0]
    d = C.iqr_case_data(shape)
    P.assert_power(d["ref_s"], "test points")
    P.assert_power(d["ref_a"], "importance points")
    assert d["cross_share"] >= 0.5
    for name in ("acqviqr", "acqimiqr"):
        ref, _, vtot = R.acqwrapper_vbmc(d["Xs"], d["vp"], d["gp"], d["st_o"][name], name)
        ok = np.isfinite(ref) & (vtot > 1e-7 * np.exp(2 * d["gp"]["post"][0]["hyp"][D]))
        assert np.mean(ok) >= P.POWER_OK


class _OracleAsDevice:
    """stands where the device does in tests/test_gpu_random_shapes._acquisition_case: the oracle's own acquisition values"""

    def acqwrapper_vbmc(self, Xs, vp, gp, st, transpose, name, _):
        name = name.replace("_vbmc", "")
        if name in ("acqviqr", "acqimiqr"):
            ais = st["ActiveImportanceSampling"]
            Kax, Ct = R.acq_is_precompute(gp, ais["Xa"])
            fs2a = np.asarray(R.gplite_pred(gp, ais["Xa"], None, None, True)[3]).reshape(ais["Xa"].shape[0], -1)
            st = dict(st, ActiveImportanceSampling=dict(ais, Kax_mat=Kax, Ctmp_mat=Ct, fs2a=fs2a))
        return R.acqwrapper_vbmc(Xs, vp, gp, st, name)[0]


def test_acquisition_sweeps_keep_their_points_inside_the_mask():
    """the derandomised examples of the two acquisition sweeps of tests/test_gpu_random_shapes.py, with the oracle in the device's place:
    the share of points inside the `ok` mask that _acquisition_case asserts holds for every one of them"""
    from tests import test_gpu_random_shapes as T

    T.test_acquisition_random_shapes(va=_OracleAsDevice())
    T.test_acquisition_random_shapes_wide(va=_OracleAsDevice())

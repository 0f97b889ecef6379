"""CPU checks on the NumPy restatement of gplite_quad (tests/_quad_ref.py), the reference the device tests of tests/test_gpu_quad.py
compare against: the 50-digit vectors of tools/mp_quad_golden.py, and the three identities that tie it to the oracle's gplite_pred and
gplogjoint.  All at the project's oracle tolerance of 1e-12, F relative and varF relative to nf_kk."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _quad_ref as Q
from tests.test_gpu_elbo import problem, relerr

TOL = 1e-12


def test_three_golden_cases_cover_the_issue():
    paths = Q.quad_golden_cases()
    assert len(paths) == 3
    meanfuns, low, zero = set(), 0, 0
    for path in paths:
        inp, gp, exp = Q.load_quad_golden(path)
        assert inp["N"] <= 12 and inp["D"] <= 3 and inp["Nstar"] <= 5
        meanfuns.add(inp["meanfun"])
        low += sum(not p["Lchol"] and np.exp(2 * p["hyp"][inp["D"] + 1]) < 1e-6 for p in gp["post"])
        zero += int(np.any(inp["sigma"] == 0))
    assert meanfuns == {0, 1, 4} and low >= 1 and zero >= 1


@pytest.mark.parametrize("path", Q.quad_golden_cases())
def test_restatement_matches_golden(path):
    inp, gp, exp = Q.load_quad_golden(path)
    F, varF = Q.gplite_quad(gp, inp["mu"], inp["sigma"], True)
    eF = relerr(F, exp["F"].T)
    eV = np.max(np.abs(varF - exp["varF"].T) / exp["nf_kk"][None, :])
    print("F rel %.2e  varF / nf_kk %.2e" % (eF, eV))
    assert relerr(Q.nf_kk(gp, inp["sigma"]), exp["nf_kk"]) < TOL
    assert eF < TOL and eV < TOL
    Fa, va = Q.gplite_quad(gp, inp["mu"], inp["sigma"], False)                # :112-119
    assert Fa.shape == (inp["Nstar"],) and relerr(Fa, exp["F_avg"]) < TOL
    assert np.max(np.abs(va - exp["varF_avg"])) < TOL * np.max(exp["nf_kk"])
    # one output, and a full Nstar x D sigma of equal rows (:27)
    F1, none = Q.gplite_quad(gp, inp["mu"], np.repeat(inp["sigma"][None, :], inp["Nstar"], axis=0), True, nargout=1)
    assert none is None and np.array_equal(F1, F)


@pytest.mark.parametrize("meanfun", [0, 1, 4])
def test_sigma_zero_is_gplite_pred(meanfun):
    """sigma = 0: tau = ell, lnnf = ln sf2, nf_kk = sf2 -- the integral against a point mass is the prediction (gplite_pred.m:74-104)."""
    gp, p = Q.mixed_gp(5, 3, 25, 3, meanfun)
    assert [q["Lchol"] for q in gp["post"]] == [True, False, True]
    Xs = 1.2 * np.random.default_rng(1).standard_normal((30, 3))
    F, varF = Q.gplite_quad(gp, Xs, np.zeros((1, 3)), True)
    _, _, fmu, fs2 = R.gplite_pred(gp, Xs, None, None, True)
    sf2 = np.array([np.exp(2 * q["hyp"][3]) for q in gp["post"]])
    assert relerr(F, fmu) < TOL
    assert np.max(np.abs(varF - np.maximum(Q.EPS, fs2)) / sf2[None, :]) < TOL


@pytest.mark.parametrize("meanfun", [0, 1, 4])
def test_component_moments_are_gplogjoint(meanfun):
    """sigma = sigma_k lambda, mu = mu_k: I_sk[s,k] and J_sjk[s,k,k] of gplogjoint at delta = 0 (gplogjoint.m:171-186,273-304)."""
    p, gp, vp, _ = problem(9, 3, 25, 4, 2, meanfun=meanfun)
    r = R.gplogjoint(vp, gp, (0, 0, 0, 0), True, True, 1, separate_K=True)
    for k in range(vp["K"]):
        sg = vp["sigma"][k] * vp["lambda"].reshape(-1)
        F, varF = Q.gplite_quad(gp, vp["mu"][:, k][None, :], sg[None, :], True)
        assert relerr(F[0], r["I_sk"][:, k]) < TOL
        # J_kk is not clamped in gplogjoint (:293); away from the clamp the two agree
        assert np.all(r["J_sjk"][:, k, k] > Q.EPS)
        assert np.max(np.abs(varF[0] - r["J_sjk"][:, k, k]) / Q.nf_kk(gp, sg)) < TOL


@pytest.mark.parametrize("name", ["acqf", "acqflog", "acqus"])
def test_wrapper_with_tiny_delta_tends_to_the_plain_wrapper(name):
    """The restated delta branch of acqwrapper_vbmc feeds the oracle's acquisition formulas: with delta -> 0 it is the oracle's wrapper."""
    p, gp, vp, _ = problem(7, 3, 30, 3, 2)
    Xs = 1.2 * np.random.default_rng(2).standard_normal((40, 3))
    st = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": True, "TolGPVar": 1e-4}
    a0, f0, v0 = R.acqwrapper_vbmc(Xs, vp, gp, st, name)
    a1, f1, v1 = Q.acqwrapper_vbmc(Xs, dict(vp, delta=np.full(3, 1e-9)), gp, st, name)
    assert relerr(f1, f0) < 1e-10 and np.allclose(a1, a0, rtol=1e-6, atol=0)
    # a real delta smooths: the variance of the integral is below the pointwise variance's prior scale, and the values differ
    a2, f2, v2 = Q.acqwrapper_vbmc(Xs, dict(vp, delta=np.array([0.3, 0.0, 0.2])), gp, st, name)
    assert not np.allclose(a2, a0, rtol=1e-3) and np.all(np.isfinite(a2)) and np.all(v2 > 0)

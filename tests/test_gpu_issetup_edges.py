"""GPU: the importance sampler's set-up and chain (vbmc_acq_is_setup, vbmc_acq_is_sample) at their widths, seams and run-out, in parity mode
against the NumPy restatements tests/_issetup_ref.py (the EDGES table) and tests/_issample_ref.py (EDGE_CASES) fed the oracle's gplite_pred.
tests/test_issetup_restatement.py and tests/test_issample_restatement.py assert, for these very tables, the margin of every draw and of
every consumed comparison, and that each case reaches the path it is named for.

Tolerances.  Xa1, rect_delta, LB, UB, idx0, x0: identical.  lnw1, fs2a1 and the seams' fmu = lnw1 + lpdf1: 1e-9 relative on the scales of
tests/test_gpu_issetup.py (fs2 on max(1, sf2)); the float64 oracle itself deviates from the same prediction carried out in np.longdouble
by 1.8e-13 (fmu) and 2.0e-14 (fs2) at N = 1136, the top of the resident range (the device: 1.9e-13 and 6.6e-14), so ten times its own
error stays below 1e-9 and the bound is 1e-9 at every seam.  Measured against the oracle: fmu 3.7e-13 and fs2 8.6e-14 at the most (N1136).
The chain: funccount equal, Xa 1e-10, logp / lnw / fs2a 1e-9 (tests/test_gpu_issample.py's assertions, called as they stand).

lpdf1.  LPDF_TOL = 3.6e-14 of tests/test_gpu_issetup.py was measured at no more than 72 components.  Here the proposal's log density of
the same points is evaluated in np.longdouble (the same formula, log-sum-exp over the 4K components); the device may deviate from that
value by ten times the float64 restatement's own deviation from it, never less than LPDF_TOL, never more than 1e-10.  Measured,
restatement / device against the long-double value, absolute (max |lpdf1| in brackets):
  R, R9, O  7.7e-16 / 1.1e-15  (5.8)     L   1.4e-15 / 1.4e-15  (10.6)    RL  1.4e-15 / 1.8e-15  (10.6)
  W   1.5e-14 / 1.5e-14  (75.3; the bound is 1.5e-13)          K   1.2e-15 / 1.4e-15  (6.5; 2048 components)
  N7 .. N1136  1.3e-15 at the most / 1.9e-15 at the most  (10.7 at the most)
Every case but W is held to LPDF_TOL.
"""
import math

import numpy as np
import pytest

from tests import _issample_ref as I
from tests import _issetup_ref as T
from tests import test_gpu_issample as CHAIN
from tests import test_gpu_issetup as SETUP

pytestmark = pytest.mark.gpu
STEP1, STEP2, LPDF_TOL = SETUP.STEP1, SETUP.STEP2, SETUP.LPDF_TOL
PRED_TOL = 1e-9
TOP = T.SEAM_NAMES[-1]                                     # N = 1136, the largest N at which inv(L') stays resident


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def device_run(c, **kw):
    if c["Nm"] == 0:                                                           # Step 1 alone: the block ends with the points
        kw.setdefault("uniforms", None)
    return SETUP.device_run(c, **kw)


def sf2_of(c):
    return np.array([np.exp(2 * p["hyp"][c["D"]]) for p in c["gp"]["post"]])


def lpdf_reference(c, ref):
    """the long-double value, the float64 restatement's deviation from it, and the device's bound"""
    ld = T.proposal_lpdf_longdouble(ref["Xa1"], c["vp"], c["gp"]["X"], c["Nvp"], c["Nbox"])
    pf = np.isfinite(ref["lpdf1"])
    assert np.array_equal(np.isfinite(ld), pf)
    own = float(np.max(np.abs(ref["lpdf1"][pf] - ld[pf])))
    return ld, own, min(max(LPDF_TOL, 10.0 * own), 1e-10)


@pytest.mark.parametrize("name", sorted(T.EDGES))
def test_edge_case_against_the_restatement(va, name):
    c, ref = T.run_case(name)
    S, W, D, step2 = c["S"], c["W"], c["D"], c["Nm"] > 0
    assert not step2 or ref["margin"] > T.DRAW_MARGIN
    d = device_run(c)
    for k in ("Xa1", "rect_delta", "LB", "UB"):
        assert np.array_equal(d[k], ref[k]), k
    for k in STEP1 + (("x0",) if step2 else ()) + (STEP2 if "Xa" in d else ()):
        assert not np.any(np.isnan(d[k])), k
    fin = np.isfinite(ref["lnw1"])
    assert np.array_equal(np.isfinite(d["lnw1"]), fin) and np.all(d["lnw1"][~fin] == -np.inf)
    pf = np.isfinite(ref["lpdf1"])
    assert np.array_equal(np.isfinite(d["lpdf1"]), pf)
    fmu = ref["fmu1"].T
    with np.errstate(invalid="ignore"):
        scale = np.maximum(1.0, np.maximum(np.where(np.isfinite(fmu), np.abs(fmu), 0.0), np.abs(ref["lpdf1"])[None, :]))
    eW = float(np.max(np.abs(d["lnw1"][fin] - ref["lnw1"][fin]) / scale[fin]))
    eF = float(np.max(np.abs(d["fs2a1"] - ref["fs2a1"]) / np.maximum(1.0, sf2_of(c))[None, :]))
    eB = float(np.max(np.abs((fmu - d["lnw1"])[fin] - np.broadcast_to(ref["lpdf1"][None, :], fin.shape)[fin]) / scale[fin]))
    ld, own, bound = lpdf_reference(c, ref)
    eP = float(np.max(np.abs(d["lpdf1"][pf] - ld[pf])))
    print("%s: lnw1 %.2e  fs2a1 %.2e  fmu - lnw1 %.2e  lpdf1 against long double: restatement %.3e device %.3e (bound %.2e, max |lpdf1| %.1f)"
          % (name, eW, eF, eB, own, eP, bound, float(np.max(np.abs(ref["lpdf1"][pf])))))
    assert eW < PRED_TOL and eF < PRED_TOL and eB < PRED_TOL
    assert eP <= bound
    if not step2:
        assert "x0" not in d and "Xa" not in d and d["funccount"] == 0 and d["state"] is not None
        return
    assert np.array_equal(d["idx0"], ref["idx0"])                              # every one of the W S draws
    assert np.array_equal(d["x0"], ref["x0"])
    if name == "O":                                                            # every start of the dead hyper-sample has zero density
        expect = np.zeros((W, S), dtype=bool)
        expect[:, 2] = True
        assert d["n_bad"] == W and np.array_equal(d["bad"], expect)
        assert "Xa" not in d and d["state"] is None and d["funccount"] == S * W and d["rounds"] == 0
    else:
        assert d["n_bad"] == 0 and not np.any(d["bad"])
        assert d["Xa"].shape == (c["Nm"], D, S) and np.all(np.isfinite(d["lnw"])) and d["funccount"] > S * W
        assert np.all(d["Xa"] >= d["LB"][None, :, None]) and np.all(d["Xa"] <= d["UB"][None, :, None])


@pytest.mark.parametrize("name", ["R", "RL", "O"])
def test_reset_weights_leave_nothing_behind(va, name):
    """the device's own idx0: a repeat-free prefix of the points that had a weight, then draws from weights of one; twice the same bits;
    the next call is untouched"""
    c, ref = T.run_case(name)
    W, Na1, D = c["W"], c["Na1"], c["D"]
    d = device_run(c)
    reset = [s for s, q in enumerate(ref["draws"]) if q["resets"]]
    assert reset == {"R": [0, 2], "RL": [0, 1], "O": [2]}[name]
    for s in reset:
        npos = ref["draws"][s]["npos"]
        idx, lw = d["idx0"][:, s], ref["lw"][:, s]
        u = c["B"][(D + 1) * Na1 + W * s:(D + 1) * Na1 + W * (s + 1)]
        assert ref["draws"][s]["resets"] == [npos] and npos < W
        if npos > 0:
            assert sorted(idx[:npos].tolist()) == sorted(np.argsort(-lw, kind="stable")[:npos].tolist())
        assert np.unique(idx[npos:]).size == W - npos
        # the first draw from weights of one: cdf = 1 .. Na1, idx = #(cdf < u Na1)
        assert idx[npos] == min(int(math.ceil(u[npos] * Na1)) - 1, Na1 - 1)
    keys = STEP1 + ("x0", "idx0", "bad") + (STEP2 if "Xa" in d else ())
    SETUP.same_bits(d, device_run(c), "second run", keys=keys)
    a, refa = T.run_case("A")
    nxt = SETUP.device_run(a)
    assert nxt["n_bad"] == 0 and np.array_equal(nxt["idx0"], refa["idx0"]) and np.array_equal(nxt["x0"], refa["x0"])
    assert np.all(np.isfinite(nxt["lnw"]))


@pytest.mark.parametrize("name", T.SEAM_NAMES)
def test_prediction_at_the_seams_against_gplite_pred(va, name):
    """one k_is_pred launch, three point tiles under both hyper-samples: fs2a1 and fmu = lnw1 + lpdf1 against the oracle's gplite_pred"""
    c, ref = T.run_case(name)
    assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False] and c["Na1"] == 48
    d = device_run(c)
    assert np.array_equal(d["Xa1"], ref["Xa1"])
    assert np.all(np.isfinite(d["lnw1"])) and np.all(np.isfinite(d["lpdf1"])) and np.all(np.isfinite(d["fs2a1"]))
    fmu_ref, fs2_ref = ref["fmu1"], ref["fs2a1"]                               # R.gplite_pred at those very points (T.setup)
    fmu = (d["lnw1"] + d["lpdf1"][None, :]).T
    sf2 = np.maximum(1.0, sf2_of(c))[None, :]
    scale = np.maximum(1.0, np.maximum(np.abs(fmu_ref), np.abs(ref["lpdf1"])[:, None]))
    eM = np.max(np.abs(fmu - fmu_ref) / scale, axis=0)
    eF = np.max(np.abs(d["fs2a1"] - fs2_ref) / sf2, axis=0)
    print("%s: N = %d, per hyper-sample (Cholesky, low-noise): fmu %s  fs2 %s" % (name, c["N"], ["%.2e" % v for v in eM], ["%.2e" % v for v in eF]))
    if name == TOP:
        lm, lf = T.gplite_pred_longdouble(c["gp"], ref["Xa1"])
        oM = float(np.max(np.abs(fmu_ref - lm) / scale))
        oF = float(np.max(np.abs(fs2_ref - lf) / sf2))
        dM = float(np.max(np.abs(fmu - lm) / scale))
        dF = float(np.max(np.abs(d["fs2a1"] - lf) / sf2))
        print(TOP + " against the long-double prediction: oracle fmu %.2e fs2 %.2e, device fmu %.2e fs2 %.2e" % (oM, oF, dM, dF))
        assert 10.0 * max(oM, oF) < PRED_TOL                                   # so that the bound below is the project's 1e-9
    assert float(np.max(eM)) < PRED_TOL and float(np.max(eF)) < PRED_TOL


def test_the_first_refused_n(va):
    """N = 1137, one more than the top of the resident range: the status from both entry points, and the call after it works"""
    from tests import _quad_ref as Q
    from vbmc_amd.acq import importance_sample_device, importance_setup_device

    gp, _ = Q.mixed_gp(1, 4, T.N_REFUSED, 1, 4)
    X = gp["X"]
    vp = {"D": 4, "K": 2, "mu": X[:2].T.copy(), "sigma": np.full(2, 0.3), "lambda": np.ones(4), "w": np.full(2, 0.5)}
    with pytest.raises(va.VbmcUnsupported):
        importance_setup_device(vp, gp, 10, 10, 4, seed=1)
    with pytest.raises(va.VbmcUnsupported):
        importance_setup_device(vp, gp, 10, 10, 0, seed=1)
    with pytest.raises(va.VbmcUnsupported):
        importance_sample_device(gp, X[:10][None, :, :], np.min(X, axis=0) - 1.0, np.max(X, axis=0) + 1.0, 4, seed=1)
    a, refa = T.run_case("A")
    nxt = SETUP.device_run(a)
    assert nxt["n_bad"] == 0 and np.array_equal(nxt["idx0"], refa["idx0"]) and np.all(np.isfinite(nxt["lnw"]))


@pytest.mark.parametrize("name", sorted(I.EDGE_CASES))
def test_chain_parity_at_the_seams(va, name):
    CHAIN.test_parity_with_the_restatement(va, name)


@pytest.mark.parametrize("name", ["H", "T"])
def test_spec_and_chunk_change_no_bit_at_the_seams(va, name):
    c, _ = I.run_case(name)
    base = CHAIN.device_run(va, c, spec=1, chunk=16)
    assert base["performed"] == base["funccount"]
    CHAIN.same_bits(base, CHAIN.device_run(va, c, spec=3, chunk=16), "spec 3")
    CHAIN.same_bits(base, CHAIN.device_run(va, c, spec=3, chunk=1), "spec 3, chunk 1")
    CHAIN.same_bits(base, CHAIN.device_run(va, c, spec=1, chunk=1), "chunk 1")


@pytest.mark.parametrize("name", ["L", "W"])
def test_device_generator_replays_at_the_limits(va, name):
    """rng_mode 0 at Na1 = 256 and at D = 32, W = 66: the same bits from the two dumps"""
    SETUP.test_device_generator_replays_through_its_dumps(va, name)

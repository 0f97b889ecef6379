"""GPU parity on randomly drawn problem shapes and flag combinations (hypothesis, derandomised): the HIP path
through the C ABI against the oracle -- the three-way cross-check of SURVEY 8c(4) with the mpmath vectors pinning
the oracle itself (tests/test_oracle_golden.py)."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from oracle import vbmc_ref as R
from tests._cases import synth_problem
from tests._pred_ref import POWER_OK, near_data_points
from tests.test_gpu_elbo import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


# VBMC_HYP_SCALE=10 multiplies the example counts for an occasional deeper sweep (the default keeps the suite at seconds)
SCALE = int(os.environ.get("VBMC_HYP_SCALE", "1"))


def half_near_data(gp, pts, seed):
    """every second row of ``pts`` replaced by a point that sees the data (tests/_pred_ref.near_data_points): drawn around the origin
    alone, the points have a cross-kernel of zero from D = 13 upwards, and a prediction is then the mean function and sf2"""
    pts = pts.copy()
    n = pts[::2].shape[0]
    pts[::2] = near_data_points(gp, n, np.random.default_rng(seed + 11))
    return pts

shape = st.tuples(st.integers(1, 8), st.integers(1, 20), st.integers(5, 60), st.integers(1, 4))


@settings(max_examples=30 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=shape, seed=st.integers(0, 10**6), flags=st.tuples(st.booleans(), st.booleans(), st.booleans(), st.booleans()),
       ns_half=st.integers(0, 20), compute_var=st.sampled_from([0, 0, 1, 2]), meanfun=st.sampled_from([0, 1, 4, 4]),
       beta=st.sampled_from([0.0, 0.0, 1.3]), grad=st.booleans())
def test_negelcbo_random_shapes(va, shape, seed, flags, ns_half, compute_var, meanfun, beta, grad):
    D, K, N, S = shape
    if not any(flags[:3]):
        flags = (True,) + flags[1:]                  # the weights-only branch (negelcbo_vbmc.m:54) is host-side, cached-stats code
    p = synth_problem(seed, D, N, K, S, meanfun=meanfun)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"], optimize=flags)
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    theta, vp = R.get_vptheta(vp)
    Ns = 2 * ns_half
    if grad and compute_var == 1:
        compute_var = 2                              # a gradient with variance needs the diagonal approximation (gplogjoint.m:28-32)
    if beta != 0.0 and compute_var == 0:
        beta = 0.0
    eps = np.random.default_rng(seed + 1).standard_normal((K, max(ns_half, 1), D))[:, :ns_half, :] if Ns > 0 else None
    ref = R.negelcbo_vbmc(theta, beta, vp, gp, Ns, grad, compute_var, eps=eps)
    out = va.negelcbo_batch(theta, beta, vp, gp, Ns, grad, compute_var, eps=eps)
    assert relerr(out["F"][0], ref["F"]) < 1e-9, (shape, flags, Ns, compute_var, meanfun, beta)
    if grad:
        assert relerr(out["dF"][:, 0], ref["dF"]) < 1e-8
    assert relerr(out["G"][0], ref["G"]) < 1e-9 and relerr(out["H"][0], ref["H"]) < 1e-9
    if compute_var:
        # varG is a difference (prior integral minus |L' \ z|^2): its error relative to the oracle grows with the condition number of
        # the kernel matrix -- and so does the oracle's own.  1e-7 up to cond(K) = 1e6, in proportion beyond (the 100x sweep reaches a
        # noise-free one-dimensional GP of 53 points, cond(K) ~ 3e7, where the product with the explicit inverse is off by 1.3e-7 and
        # the substitution by 2.4e-7: round 5, `profiles/r05_var.md`)
        condK = max((np.linalg.cond(q["L"]) ** 2 if q["Lchol"] else np.linalg.cond(q["L"])) for q in gp["post"])
        assert relerr(out["varG"][0], ref["varG"]) < 1e-7 * max(1.0, condK / 1e6), condK


wide = st.tuples(st.integers(1, 32), st.integers(1, 200), st.integers(5, 220), st.integers(1, 3))


@settings(max_examples=8 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=wide, seed=st.integers(0, 10**6), ns_half=st.integers(0, 10), compute_var=st.sampled_from([0, 0, 2]), grad=st.booleans())
def test_negelcbo_random_shapes_wide(va, shape, seed, ns_half, compute_var, grad):
    """The same comparison over the whole supported range of D (<= 32), K (MFMA kernels up to 128 incl. the two-wave split, the
    VALU kernel beyond) and N of a few hundred: every padded-dimension / k-tile instantiation is reachable from here."""
    D, K, N, S = shape
    p = synth_problem(seed, D, N, K, S, meanfun=4)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4, noisefun=p["noisefun"], s2=p["s2"])
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    theta, vp = R.get_vptheta(vp)
    Ns = 2 * ns_half
    eps = np.random.default_rng(seed + 1).standard_normal((K, max(ns_half, 1), D))[:, :ns_half, :] if Ns > 0 else None
    # documented limit: the variance gradient keeps five T-vectors in LDS
    too_big = grad and compute_var == 2 and 5 * theta.size + 2 * (S + K) + 1024 + 8 > 20480
    if too_big:
        with pytest.raises(va.VbmcUnsupported):
            va.negelcbo_batch(theta, 0.0, vp, gp, Ns, grad, compute_var)
        return
    ref = R.negelcbo_vbmc(theta, 0.0, vp, gp, Ns, grad, compute_var, eps=eps)
    out = va.negelcbo_batch(theta, 0.0, vp, gp, Ns, grad, compute_var, eps=eps)
    assert relerr(out["G"][0], ref["G"]) < 1e-9 and relerr(out["H"][0], ref["H"]) < 1e-9, (shape, Ns, compute_var)
    # F = -(G + H) (beta = 0): 1e-9 of the terms it is made of, which is 1e-9 of F itself unless they cancel (the 100x sweep reaches
    # D = K = 1, N = 32, where |G| + |H| = 1.3 |F| and F is off by 1.16e-9 with G and H each inside 1e-9)
    assert abs(out["F"][0] - ref["F"]) < 1e-9 * max(abs(ref["F"]), abs(ref["G"]) + abs(ref["H"]), 1e-300)
    if grad:
        assert relerr(out["dF"][:, 0], ref["dF"]) < 1e-8, (shape, Ns, compute_var)
    if compute_var:
        assert relerr(out["varG"][0], ref["varG"]) < 1e-6


@settings(max_examples=15 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 8), st.integers(5, 70), st.integers(1, 4)), seed=st.integers(0, 10**6),
       meanfun=st.sampled_from([0, 1, 4]), nstar=st.integers(1, 90), noisy=st.booleans())
def test_gp_post_pred_random_shapes(va, shape, seed, meanfun, nstar, noisy):
    D, N, S = shape
    p = synth_problem(seed, D, N, 2, S, meanfun=meanfun, noisy=noisy)
    ref = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    gp = va.gplite_post(p["hyp"], p["X"], p["y"], 1, meanfun, p["noisefun"], p["s2"])
    for a, b in zip(gp["post"], ref["post"]):
        assert a["Lchol"] == b["Lchol"] and a["sn2_mult"] == b["sn2_mult"]
        assert relerr(a["alpha"], b["alpha"]) < 1e-8
    Xs = half_near_data(ref, 1.3 * np.random.default_rng(seed + 2).standard_normal((nstar, D)), seed)
    r_d = va.gplite_pred(gp, Xs, None, None, True)
    r_o = R.gplite_pred(ref, Xs, None, None, True)
    sf2 = np.exp(2 * ref["post"][0]["hyp"][D])
    assert relerr(np.asarray(r_d[2]).reshape(-1), np.asarray(r_o[2]).reshape(-1)) < 1e-8
    assert np.max(np.abs(np.asarray(r_d[3]).reshape(-1) - np.asarray(r_o[3]).reshape(-1))) < 1e-8 * sf2


@settings(max_examples=20 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 8), st.integers(5, 60), st.integers(1, 3), st.integers(1, 12)), seed=st.integers(0, 10**6),
       nstar=st.integers(1, 60), na=st.integers(1, 40), name=st.sampled_from(["acqf", "acqflog", "acqus", "acqfsn2", "acqviqr", "acqimiqr"]))
def test_acquisition_random_shapes(va, shape, seed, nstar, na, name):
    _acquisition_case(va, shape, seed, nstar, na, name)


@settings(max_examples=5 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 32), st.integers(5, 300), st.integers(1, 3), st.integers(1, 60)), seed=st.integers(0, 10**6),
       nstar=st.integers(1, 600), na=st.integers(1, 256), name=st.sampled_from(["acqf", "acqfsn2", "acqviqr", "acqviqr", "acqimiqr"]))
def test_acquisition_random_shapes_wide(va, shape, seed, nstar, na, name):
    """Up to 256 importance points (all 16 accumulator-tile instantiations of k_acq_iqr, the > 64 KB LDS variants), several
    128-point workgroups, D up to 32, training sets of a few hundred points."""
    _acquisition_case(va, shape, seed, nstar, na, name)


def _acquisition_case(va, shape, seed, nstar, na, name):
    D, N, S, K = shape
    p = synth_problem(seed, D, N, K, S)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4)
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    rng = np.random.default_rng(seed + 3)
    Xs = half_near_data(gp, 1.3 * rng.standard_normal((nstar, D)), seed)
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    gp = dict(gp, X_rescaled=p["X"] / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    st_ = {"ymax": float(np.max(p["y"])), "VarianceRegularizedAcqFcn": False, "TolGPVar": 1e-4, "gplengthscale": gl}
    if name in ("acqviqr", "acqimiqr"):
        Xa = half_near_data(gp, 1.2 * rng.standard_normal((na, D)), seed + 1)
        Kax, Ct = R.acq_is_precompute(gp, Xa)
        fs2a = np.asarray(R.gplite_pred(gp, Xa, None, None, True)[3]).reshape(na, -1)
        lnw = np.zeros((S, na)) if name == "acqviqr" else 0.5 * rng.standard_normal((S, na))
        st_o = dict(st_, ActiveImportanceSampling={"Xa": Xa, "Kax_mat": Kax, "Ctmp_mat": Ct, "fs2a": fs2a, "lnw": lnw})
        st_d = dict(st_, ActiveImportanceSampling={"Xa": Xa, "lnw": lnw})
    else:
        st_o = st_d = st_
    ref, _, vtot = R.acqwrapper_vbmc(Xs, vp, gp, st_o, name)
    acq = va.acqwrapper_vbmc(Xs, vp, gp, st_d, False, name + "_vbmc", None)
    sf2 = np.exp(2 * gp["post"][0]["hyp"][D])
    ok = np.isfinite(ref) & (vtot > 1e-7 * sf2)
    # the inputs keep their power: at most a tenth of the points (one, for a handful of points) fall outside the mask.  The derandomised
    # examples are checked against this on the CPU, with the oracle in the device's place (tests/test_pred_restatement.py)
    assert ok.size - np.sum(ok) <= max(1, (1 - POWER_OK) * ok.size), (shape, name, np.mean(ok))
    # fs2 = kss - |V|^2 cancels near training inputs: both implementations carry an absolute error ~ 1e-12 sf2 there, i.e. a
    # relative one of 1e-12 sf2 / vtot in everything proportional to vtot (found by the 10x sweep: D=1, N=36, vtot = 1e-5 sf2)
    rt = 1e-7 + 1e-11 * sf2 / np.maximum(vtot[ok], 1e-300)
    if name in ("acqflog", "acqviqr", "acqimiqr"):
        assert np.all(np.abs(acq[ok] - ref[ok]) < rt * (1 + np.abs(ref[ok]))), (shape, name)
    else:
        assert np.all(np.abs(acq[ok] - ref[ok]) <= rt * np.abs(ref[ok]) + 1e-300), (shape, name)


@settings(max_examples=20 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 8), st.integers(3, 80), st.integers(1, 6)), seed=st.integers(0, 10**6),
       meanfun=st.sampled_from([0, 1, 4]), noisefun=st.sampled_from([(1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 0, 1), (1, 2, 1)]))
def test_nlz_random_shapes(va, shape, seed, meanfun, noisefun):
    from tests.test_gpu_nlz import make_gp

    D, N, B = shape
    gp, draw = make_gp(np.random.default_rng(seed), N, D, meanfun, noisefun)
    H = np.stack([draw() for _ in range(B)], axis=1)
    nlZ, dnlZ = va.gplite_nlZ(H, gp) if B > 1 else va.gplite_nlZ(H[:, 0], gp)
    nlZ = np.atleast_1d(nlZ)
    dnlZ = np.asarray(dnlZ).reshape(H.shape[0], -1)
    for b in range(B):
        f, g = R.gplite_nlZ(H[:, b], gp)
        assert abs(nlZ[b] - f) < 1e-9 * max(1.0, abs(f)), (shape, meanfun, noisefun)
        assert relerr(dnlZ[:, b], g) < 1e-7, (shape, meanfun, noisefun, relerr(dnlZ[:, b], g))


@settings(max_examples=5 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 32), st.integers(5, 420), st.integers(1, 3)), seed=st.integers(0, 10**6),
       meanfun=st.sampled_from([0, 1, 4]), nstar=st.integers(1, 400), noisy=st.booleans(), rank1=st.booleans())
def test_gp_side_random_shapes_wide(va, shape, seed, meanfun, nstar, noisy, rank1):
    """gplite_post / gplite_pred / rank-one append / gplite_nlZ over the supported range of D (padded kernel instantiations up to
    32) and training-set sizes of a few hundred (several 64 x 64 tiles, several resident row groups in the prediction kernel)."""
    from tests.test_gpu_nlz import make_gp

    D, N, S = shape
    p = synth_problem(seed, D, N, 2, S, meanfun=meanfun, noisy=noisy)
    ref = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    gp = va.gplite_post(p["hyp"], p["X"], p["y"], 1, meanfun, p["noisefun"], p["s2"])
    for a, b in zip(gp["post"], ref["post"]):
        assert a["Lchol"] == b["Lchol"] and relerr(a["alpha"], b["alpha"]) < 1e-7 and relerr(a["L"], b["L"]) < 1e-8
    if rank1 and not noisy:
        xs = 1.2 * np.random.default_rng(seed + 5).standard_normal(D)
        gp = va.gplite_post_rank1(gp, xs, 0.3, need_L=False)
        ref = R.gplite_post_rank1(ref, xs, 0.3)
        for a, b in zip(gp["post"], ref["post"]):
            assert relerr(a["alpha"], b["alpha"]) < 1e-6
    Xs = half_near_data(ref, 1.3 * np.random.default_rng(seed + 2).standard_normal((nstar, D)), seed)
    r_d = va.gplite_pred(gp, Xs, None, None, True)
    r_o = R.gplite_pred(ref, Xs, None, None, True)
    sf2 = np.exp(2 * ref["post"][0]["hyp"][D])
    assert relerr(np.asarray(r_d[2]).reshape(-1), np.asarray(r_o[2]).reshape(-1)) < 1e-7
    assert np.max(np.abs(np.asarray(r_d[3]).reshape(-1) - np.asarray(r_o[3]).reshape(-1))) < 1e-7 * sf2
    # marginal likelihood and gradient at the same sizes
    gpn, draw = make_gp(np.random.default_rng(seed + 9), N, D, meanfun, (1, 0, 0))
    H = np.stack([draw() for _ in range(2)], axis=1)
    nlZ, dnlZ = va.gplite_nlZ(H, gpn)
    for b in range(2):
        f, g = R.gplite_nlZ(H[:, b], gpn)
        assert abs(nlZ[b] - f) < 1e-9 * max(1.0, abs(f)) and relerr(dnlZ[:, b], g) < 1e-6, (shape, meanfun)


@settings(max_examples=5 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 20), st.integers(1, 128), st.integers(5, 150), st.integers(1, 3)), seed=st.integers(0, 10**6),
       ns_half=st.integers(1, 12), grad=st.booleans(), R_=st.sampled_from([2, 48, 130]))
def test_negelcbo_batched_wide(va, shape, seed, ns_half, grad, R_):
    """R restarts in one call (sieve batch / lock-step chains): few (one stream), and enough of them that the log joint moves to
    the second stream beside the entropy kernel and takes its MFMA form; three distinct thetas repeated, one shared set of draws."""
    D, K, N, S = shape
    p = synth_problem(seed, D, N, K, S, meanfun=4)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4, noisefun=p["noisefun"], s2=p["s2"])
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    theta, vp = R.get_vptheta(vp)
    rng = np.random.default_rng(seed + 4)
    base = [theta + 0.05 * rng.standard_normal(theta.size) for _ in range(3)]
    cols = [base[r % 3] for r in range(R_)]
    Th = np.asfortranarray(np.stack(cols, axis=1))
    Ns = 2 * ns_half
    eps = rng.standard_normal((K, ns_half, D))
    refs = []
    for b in base:
        refs.append(R.negelcbo_vbmc(b, 0.0, vp, gp, Ns, grad, 0, eps=eps))
    out = va.negelcbo_batch(Th, 0.0, vp, gp, Ns, grad, 0, eps=eps, eps_shared=True)
    for r in range(R_):
        ref = refs[r % 3]
        assert relerr(out["F"][r], ref["F"]) < 1e-9, (shape, R_, r)
        if grad:
            assert relerr(out["dF"][:, r], ref["dF"]) < 1e-8, (shape, R_, r)
    # identical columns give identical bits (fixed-order reductions)
    assert out["F"][0] == out["F"][3 % R_] or R_ < 4


@settings(max_examples=3 * SCALE, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(shape=st.tuples(st.integers(1, 12), st.integers(2, 70), st.integers(8, 90), st.integers(1, 3)), seed=st.integers(0, 10**6),
       ns_half=st.integers(2, 30), flags=st.sampled_from([(1, 1, 1, 1), (1, 1, 1, 0), (1, 1, 0, 1)]), chains=st.sampled_from([1, 2, 5]))
def test_device_adam_random_shapes(va, shape, seed, ns_half, flags, chains):
    """The on-device optimiser loop (Adam update folded into the next k_prep, stopping test every 20 iterations) against the host
    loop of utils/fminadam.m driving the same device objective with the same per-iteration seeds: same stopping iteration, same
    iterates -- for random shapes, warm-up style flag sets (weights fixed) and several chains in lock-step."""
    D, K, N, S = shape
    p = synth_problem(seed, D, N, K, S, meanfun=4)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4, noisefun=p["noisefun"], s2=p["s2"])
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"], optimize=flags)
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    opts = dict(TolLength=1e-6, TolWeight=1e-2, TolConLoss=0.01, WeightPenalty=0.1)
    vpb, tb = R.vpbounds(vp, gp, opts)
    theta, vpb = R.get_vptheta(vpb)
    Ns, MaxIter, sd = 2 * ns_half, 60, seed % 1000
    X0 = np.asfortranarray(np.stack([theta + 0.03 * c for c in range(chains)], axis=1))
    xd, fd, xtd, ftd, itd = va.fminadam_device(X0, 0, vpb, gp, Ns, tb, 1e-3, MaxIter, seed=sd)
    c = chains - 1                      # compare the last chain with a host loop of its own
    it = {"n": 0}

    def fun(x):
        it["n"] += 1
        Th = X0.copy()
        Th[:, c] = x                    # same restart index -> same device RNG stream (keyed by seed, restart, component, sample)
        r = va.negelcbo_batch(Th, 0, vpb, gp, Ns, True, 0, tb, seed=sd + it["n"])
        return float(r["F"][c]), r["dF"][:, c].copy()

    xh, fh, xth, fth, ith = va.fminadam(fun, X0[:, c].copy(), None, None, 1e-3, MaxIter)
    assert int(itd[c]) == ith, (shape, flags, chains)
    # Adam's update m / (sqrt(v) + 1.5e-8) amplifies last-bit differences (device pow / exp / sqrt vs NumPy's) wherever a gradient
    # component is ~ 0; over 60 iterations the two trajectories stay together to ~ 1e-7 (1e-9 in the fixed case of
    # tests/test_gpu_optimize.py), far below anything the stopping rule reads
    assert relerr(ftd[c], fth) < 1e-5 and relerr(xtd[c], xth) < 1e-5, (shape, flags, chains)

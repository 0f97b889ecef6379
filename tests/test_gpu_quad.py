"""GPU parity: gplite_quad (vbmc_gp_quad) and the vp.delta branch of the acquisition sweep (vbmc_acq_eval_delta) against the NumPy
restatement tests/_quad_ref.py, at the tolerances of tests/test_gpu_gplite.py::test_pred_many_points_few_samples -- 1e-9 relative on F,
1e-9 nf_kk absolute on varF -- and against the 50-digit vectors of tools/mp_quad_golden.py at 1e-11.

The shapes sit on the kernels' edges: one point tile and less, N no multiple of 16, the two shapes whose tile block is smaller than the
per-wave scratch that reuses it (D = 13, N = 16: two resident tiles; D = 21, N = 20: one), several row tiles, and N = 1264 for the slab
form.  Every GP with S = 3 mixes Cholesky samples with a low-noise one (L = -inv(K + sn2 I)).

The low-noise sample's rounding error is that of z' inv(K + sn2 I) z, eps N |z|' |inv| |z|, whatever evaluates it; a case is admitted only
if that figure, computed here from the reference's own factors, is below a tenth of the tolerance (``_conditioned``), so that what the
comparison measures is the quadrature pass."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _quad_ref as Q
from tests._cases import relerr
from tests._pred_ref import near_data_points
from tests.test_gpu_elbo import problem

pytestmark = pytest.mark.gpu

SHAPES = [(1, 10, 1), (3, 37, 50), (5, 48, 17), (13, 16, 33), (21, 20, 40), (10, 130, 100)]     # D, N, Nstar


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def _sigma(D, seed):
    sg = 0.1 + 0.4 * np.random.default_rng(seed).random(D)
    sg[::3] = 0.0                                   # zero entries: no smoothing along those coordinates
    if D == 1:
        sg[0] = 0.3
    return sg


def _conditioned(gp, mu, sigma):
    """eps N |z|' |inv(K + sn2 I)| |z| / nf_kk of the low-noise samples (see the module docstring)."""
    N, D = gp["X"].shape
    worst = 0.0
    for s, post in enumerate(gp["post"]):
        if post["Lchol"]:
            continue
        one = dict(gp, post=[post])
        F, _ = Q.gplite_quad(one, mu, sigma, True, nargout=1)
        tau = np.sqrt(sigma ** 2 + np.exp(post["hyp"][:D]) ** 2)
        lnnf = 2 * post["hyp"][D] + np.sum(post["hyp"][:D]) - np.sum(np.log(tau))
        z = np.exp(lnnf - 0.5 * np.sum(((mu[:, None, :] - gp["X"][None, :, :]) / tau) ** 2, axis=2))
        worst = max(worst, np.max(np.einsum("in,nm,im->i", z, np.abs(post["L"]), z)) * N * Q.EPS / Q.nf_kk(one, sigma)[0])
    return worst


def _case(D, N, Nstar, S, meanfun, seed=31):
    gp, p = Q.mixed_gp(seed, D, N, S, meanfun)
    rng = np.random.default_rng(seed + 1)
    mu = 1.3 * rng.standard_normal((Nstar, D))
    if Nstar >= 3:
        mu[-2:] = gp["X"][:2] + 1e-3                # two points beside the data: varF cancels to a small fraction of nf_kk
    sg = _sigma(D, seed)
    if D >= 13:
        # 1.3 N(0, I) around the inputs has a cross term of zero from D = 13 upwards: every second point sits near a training input on the
        # quadrature's scale tau (the smallest over the hyper-samples, so that each of them sees it), z / nf between 1e-2 and 1
        tau = np.min(np.sqrt(sg[None, :] ** 2 + np.stack([np.exp(q["hyp"][:D]) for q in gp["post"]]) ** 2), axis=0)
        near = mu[:(Nstar - 2 if Nstar >= 3 else Nstar):2]        # (the last two rows are planted from Nstar = 3)
        near[:] = near_data_points(gp, near.shape[0], np.random.default_rng(seed + 2), lo=1e-2, scale=tau)
    assert _conditioned(gp, mu, sg) < 1e-10
    return gp, mu, sg


def _check(va, gp, mu, sg, tolF=1e-9, tolV=1e-9):
    nfkk = Q.nf_kk(gp, sg)
    S = len(gp["post"])
    Fr, Vr = Q.gplite_quad(gp, mu, sg[None, :], True)
    F, V = va.gplite_quad(gp, mu, sg, True)
    assert F.shape == Fr.shape == (mu.shape[0], S) and V.shape == Vr.shape
    eF, eV = relerr(F, Fr), np.max(np.abs(V - Vr) / nfkk[None, :])
    print("ssflag=1: F rel %.2e  varF / nf_kk %.2e" % (eF, eV))
    assert eF < tolF and eV < tolV
    assert np.all(V >= Q.EPS)
    Fa_r, Va_r = Q.gplite_quad(gp, mu, sg[None, :], False)
    Fa, Va = va.gplite_quad(gp, mu, sg, False)
    assert np.asarray(Fa).shape == np.asarray(Fa_r).shape
    assert relerr(Fa, Fa_r) < tolF and np.max(np.abs(Va - Va_r)) < tolV * np.max(nfkk)
    F1 = va.gplite_quad(gp, mu, np.repeat(sg[None, :], mu.shape[0], axis=0), True, nargout=1)     # equal rows collapse to the row
    assert np.array_equal(F1, F)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_quad_matches_restatement(va, shape, S):
    D, N, Nstar = shape
    meanfun = (4, 1, 0)[(D + S) % 3]
    gp, mu, sg = _case(D, N, Nstar, S, meanfun)
    if S == 3:
        assert [p["Lchol"] for p in gp["post"]] == [True, False, True]
    _check(va, gp, mu, sg)


@pytest.mark.parametrize("meanfun", [0, 1, 4])
def test_quad_mean_functions(va, meanfun):
    gp, mu, sg = _case(4, 30, 21, 3, meanfun, seed=37)
    _check(va, gp, mu, sg)


def test_quad_slab_form(va):
    """N = 1264: beyond what the resident-tile kernels hold, the variance comes from slab solves (k_pred_slab on k_quad_ks's matrix)."""
    gp, mu, sg = _case(4, 1264, 20, 1, 4, seed=41)
    _check(va, gp, mu, sg)


@pytest.mark.parametrize("path", Q.quad_golden_cases())
def test_quad_golden(va, path):
    inp, gp, exp = Q.load_quad_golden(path)
    F, V = va.gplite_quad(gp, inp["mu"], inp["sigma"], True)
    eF, eV = relerr(F, exp["F"].T), np.max(np.abs(V - exp["varF"].T) / exp["nf_kk"][None, :])
    print("golden: F rel %.2e  varF / nf_kk %.2e" % (eF, eV))
    assert eF < 1e-11 and eV < 1e-11
    Fa, Va = va.gplite_quad(gp, inp["mu"], inp["sigma"], False)
    assert relerr(Fa, exp["F_avg"]) < 1e-11 and np.max(np.abs(Va - exp["varF_avg"])) < 1e-11 * np.max(exp["nf_kk"])


def test_sigma_zero_is_the_device_prediction(va):
    gp, mu, _ = _case(5, 48, 40, 3, 4)
    F, V = va.gplite_quad(gp, mu, np.zeros(5), True)
    _, _, fmu, fs2 = va.gplite_pred(gp, mu, None, None, True)
    sf2 = np.array([np.exp(2 * p["hyp"][5]) for p in gp["post"]])
    assert relerr(F, fmu) < 1e-9
    assert np.max(np.abs(V - np.maximum(Q.EPS, fs2)) / sf2[None, :]) < 1e-9


@pytest.mark.parametrize("meanfun", [1, 4])
def test_component_moments_are_the_device_log_joint(va, meanfun):
    """mu = mu_k, sigma = sigma_k lambda: I_sk[s,k] and J_sjk[s,k,k] of the device's expected log joint (full variance)."""
    p, gp, vp, theta = problem(9, 3, 40, 4, 3, meanfun=meanfun)
    out = va.negelcbo_vbmc(theta, 0, vp, gp, 0, 0, 1, nargout=11)
    I_sk, J_sjk = out[9], out[10]
    for k in range(vp["K"]):
        sg = vp["sigma"][k] * vp["lambda"].reshape(-1)
        F, V = va.gplite_quad(gp, vp["mu"][:, k][None, :], sg, True)
        nfkk = Q.nf_kk(gp, sg)
        assert relerr(F[0], I_sk[:, k]) < 1e-9
        assert np.all(J_sjk[:, k, k] > Q.EPS) and np.max(np.abs(V[0] - J_sjk[:, k, k]) / nfkk) < 1e-9


def _acq_setup(seed, D, N, K, S):
    p, gp, vp, _ = problem(seed, D, N, K, S)
    hyp = np.stack([q["hyp"] for q in gp["post"]], axis=1)
    hyp[D + 1, :] = np.log(0.03)
    gp = R.gplite_post(hyp, gp["X"], gp["y"], meanfun=gp["meanfun"])
    rng = np.random.default_rng(seed + 100)
    Xs = np.vstack([1.2 * rng.standard_normal((150, D)), gp["X"][:20] + 1e-3 * rng.standard_normal((20, D)), gp["X"][:5]])
    st = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": True, "TolGPVar": 1e-4}
    delta = 0.05 + 0.2 * rng.random(D)
    delta[0] = 0.0
    return gp, dict(vp, delta=delta), Xs, st, rng


@pytest.mark.parametrize("name", ["acqf", "acqflog", "acqus"])
def test_acq_delta_matches_restated_wrapper(va, name):
    D = 4
    gp, vp, Xs, st, rng = _acq_setup(7, D, 60, 5, 3)
    outside = rng.random(Xs.shape[0]) < 0.1
    ref, fbar_r, vtot_r = Q.acqwrapper_vbmc(Xs, vp, gp, st, name, outside)
    acq, fbar, vtot = va.acqwrapper_vbmc(Xs, vp, gp, st, False, name + "_vbmc", None, outside=outside, nargout=3, delta_quad=True)
    assert np.array_equal(np.isinf(acq), outside)
    ok = ~outside
    assert relerr(fbar, fbar_r) < 1e-10
    # tests/test_gpu_acq.py's tolerance expression, on the scale of the quadrature's prior variance nf_kk
    sf2 = np.max(Q.nf_kk(gp, vp["delta"]))
    assert np.max(np.abs(vtot - vtot_r)) < 1e-9 * sf2
    dv = 1e-9 * sf2
    sel = ok & (vtot_r > 1e-7 * sf2)
    assert sel.sum() > 100
    amp = (st["TolGPVar"] * (vtot_r < st["TolGPVar"]) / vtot_r**2 + 1.0 / vtot_r) * dv
    if name == "acqflog":
        assert np.all(np.abs(acq[sel] - ref[sel]) <= 1e-9 * (1 + np.abs(ref[sel])) + amp[sel])
    else:
        assert np.all(np.abs(acq[sel] - ref[sel]) <= (1e-9 + amp[sel]) * np.abs(ref[sel]) + 1e-300)
    # the smoothing is real: the plain sweep gives other values
    plain = va.acqwrapper_vbmc(Xs, dict(vp, delta=None), gp, st, False, name + "_vbmc", None, outside=outside)
    assert not np.allclose(plain[ok], acq[ok], rtol=1e-6)
    accT = va.acqwrapper_vbmc(Xs[:7].T, vp, gp, st, True, name + "_vbmc", None, delta_quad=True)
    assert accT.shape == (1, 7) and np.array_equal(accT.reshape(-1), va.acqwrapper_vbmc(Xs[:7], vp, gp, st, False, name + "_vbmc", None, delta_quad=True))


def test_acqfsn2_delta_and_sharded_form(va):
    D = 5
    gp, vp, Xs, st, rng = _acq_setup(9, D, 80, 6, 3)
    gl = np.exp(np.mean(np.stack([p["hyp"][:D] for p in gp["post"]], axis=1), axis=1))
    gp = dict(gp, X_rescaled=gp["X"] / gl[None, :], sn2new=0.01 + 0.1 * rng.random(80))
    st = dict(st, gplengthscale=gl, VarianceRegularizedAcqFcn=False)
    Xs = Xs[:150]
    ref, _, vtot_r = Q.acqwrapper_vbmc(Xs, vp, gp, st, "acqfsn2")
    acq = va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqfsn2_vbmc", None, delta_quad=True)
    assert relerr(acq, ref) < 1e-8
    # sharded: every rank evaluates its points i = rank (mod world); the gathered vector agrees with the local one to rounding
    # (sq_dist centres on the mean of the points it is given, hence per shard) and picks the same point
    world = 3
    full = np.full(Xs.shape[0], np.nan)
    for rank in range(world):
        def allgather(v, idx, n, rank=rank):
            full[idx] = v
            return full
        va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqfsn2_vbmc", None, shard=(rank, world, allgather), delta_quad=True)
    assert np.allclose(full, acq, rtol=1e-11, atol=0) and int(np.argmin(full)) == int(np.argmin(acq))


def test_refusals(va):
    from vbmc_amd._lib import VBMC_ERR_INVALID, f64, ptr
    from vbmc_amd.elbo import default_engine
    from vbmc_amd.gplite import _device_gp_with_noise

    gp, vp, Xs, st, rng = _acq_setup(3, 3, 20, 2, 2)
    mu = Xs[:6]
    sg = np.abs(rng.standard_normal((6, 3)))
    with pytest.raises(va.VbmcUnsupported):                       # a sigma row per point
        va.gplite_quad(gp, mu, sg)
    eng = default_engine()
    dgp = _device_gp_with_noise(eng, gp)
    F = np.zeros((6, 2), order="F")
    m_, s_ = f64(mu), f64(sg)
    assert eng.ctx.lib.vbmc_gp_quad(eng.ctx.h, dgp.h, 6, ptr(m_), ptr(s_), 6, 1, ptr(F), None) == 4      # VBMC_ERR_UNSUPPORTED
    with pytest.raises(va.VbmcUnsupported):                       # the IQR functions with delta
        va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqviqr_vbmc", None, delta_quad=True)
    with pytest.raises(va.VbmcUnsupported):                       # the default keeps refusing
        va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqf_vbmc", None)
    # an all-zero delta handed to vbmc_acq_eval_delta itself
    X_ = f64(Xs)
    K = vp["K"]
    a = [f64(np.asarray(vp[k], dtype=np.float64)) for k in ("mu", "sigma", "lambda", "w")]
    out = [np.zeros(X_.shape[0]) for _ in range(3)]
    z = f64(np.zeros(3))
    rc = eng.ctx.lib.vbmc_acq_eval_delta(eng.ctx.h, dgp.h, X_.shape[0], ptr(X_), 0, K, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), 0.0, 0, 0.0,
                                         None, None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(z))
    assert rc == VBMC_ERR_INVALID
    rc = eng.ctx.lib.vbmc_acq_eval_delta(eng.ctx.h, dgp.h, X_.shape[0], ptr(X_), 10, K, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), 0.0, 0, 0.0,
                                         None, None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(f64(np.array([0.1, 0.0, 0.2]))))
    assert rc == 4
    # an all-zero vp.delta is the plain sweep (acqwrapper_vbmc.m:12), with or without delta_quad
    p0 = va.acqwrapper_vbmc(Xs, dict(vp, delta=np.zeros(3)), gp, st, False, "acqf_vbmc", None, delta_quad=True)
    assert np.array_equal(p0, va.acqwrapper_vbmc(Xs, dict(vp, delta=None), gp, st, False, "acqf_vbmc", None))

"""GPU: the device-resident MCMC of the IMIQR importance sampler (vbmc_acq_is_sample) against the NumPy restatement
tests/_issample_ref.py::sample fed the oracle's gplite_pred, given the same uniforms (parity mode), on the cases of that file.

Tolerances.  Xa: 1e-10 relative (to the box), the figure tests/test_gpu_slice.py holds samples to given identical decisions -- guarded by
the 1e-6 margin tests/test_issample_restatement.py asserts for this very table.  logp, lnw, fs2a: 1e-9 relative (fs2a on the scale
max(1, sf2)), the prediction's tolerance against the oracle in tests/test_gpu_gplite.py:43-44."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _issample_ref as I

pytestmark = pytest.mark.gpu
KEYS = ("Xa", "logp", "lnw", "fs2a")


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def device_run(va, c, **kw):
    from vbmc_amd.acq import importance_sample_device

    args = dict(thin=c["thin"], uniforms=c["U"], spec=1)
    args.update(kw)
    gp = args.pop("gp", c["gp"])
    x0 = args.pop("x0", c["x0"])
    LB, UB = args.pop("LB", c["LB"]), args.pop("UB", c["UB"])
    Nm = args.pop("Nm", c["Nm"])
    return importance_sample_device(gp, x0, LB, UB, Nm, **args)


def same_bits(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["funccount"] == b["funccount"], what


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_parity_with_the_restatement(va, name):
    c, ref = I.run_case(name)
    assert ref["margin"] > I.MARGIN
    d = device_run(va, c)
    span = (c["UB"] - c["LB"])[None, :, None]
    S, Nm = c["S"], c["Nm"]
    eX = float(np.max(np.abs(d["Xa"] - ref["Xa"]) / span))
    eL = float(np.max(np.abs(d["logp"] - ref["logp"]) / np.maximum(1.0, np.abs(ref["logp"]))))
    fmu = np.zeros((S, Nm))
    fs2 = np.zeros((Nm, S))
    for s in range(S):
        _, _, fm, f2 = R.gplite_pred(c["gp"], ref["Xa"][:, :, s], None, None, True)
        fmu[s] = np.asarray(fm).reshape(Nm, -1)[:, s]
        fs2[:, s] = np.asarray(f2).reshape(Nm, -1)[:, s]
    lnw = fmu - ref["logp"]
    sf2 = np.array([np.exp(2 * p["hyp"][c["D"]]) for p in c["gp"]["post"]])
    eW = float(np.max(np.abs(d["lnw"] - lnw) / np.maximum(1.0, np.maximum(np.abs(fmu), np.abs(ref["logp"])))))
    eF = float(np.max(np.abs(d["fs2a"] - fs2) / np.maximum(1.0, sf2)[None, :]))
    print("%s: Xa %.2e  logp %.2e  lnw %.2e  fs2a %.2e  funccount %d / %d  rounds %d" % (name, eX, eL, eW, eF, d["funccount"], ref["funccount"], d["rounds"]))
    assert d["funccount"] == ref["funccount"]
    assert eX < 1e-10
    assert eL < 1e-9 and eW < 1e-9 and eF < 1e-9
    assert np.all(d["Xa"] >= c["LB"][None, :, None]) and np.all(d["Xa"] <= c["UB"][None, :, None])
    if name == "E":
        assert ref["outside"] > 0


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_spec_and_chunk_change_no_bit(va, name):
    c, _ = I.run_case(name)
    base = device_run(va, c, spec=1, chunk=16)
    assert base["performed"] == base["funccount"]
    perf = [base["performed"]]
    for spec in (2, 3, 4):
        r = device_run(va, c, spec=spec)
        same_bits(base, r, "spec %d" % spec)
        perf.append(r["performed"])
        assert r["rounds"] <= base["rounds"]
    assert perf[0] < perf[1] <= perf[2] <= perf[3], perf
    for chunk in (1, 5):
        same_bits(base, device_run(va, c, spec=3, chunk=chunk), "chunk %d" % chunk)


def test_device_generator_replays_through_its_dump(va):
    from vbmc_amd.acq import importance_sample_rng_dump

    c, _ = I.run_case("B")
    a = device_run(va, c, uniforms=None, seed=20240607, spec=3)
    U = importance_sample_rng_dump(20240607, c["S"], c["H"], c["M"])
    b = device_run(va, c, uniforms=U, spec=3)
    same_bits(a, b, "replay")
    assert a["performed"] == b["performed"] and a["rounds"] == b["rounds"]


def test_returned_state_is_the_state_of_the_downloaded_arrays(va):
    from tests import _acqsearch_iqr_ref as Q

    c, _ = I.run_case("C")
    d = device_run(va, c, spec=3)
    gp = c["gp"]
    D, N = c["D"], c["N"]
    rng = np.random.default_rng(5)
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    gp2 = dict(gp, X_rescaled=gp["X"] / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    eng = va.default_engine()
    from vbmc_amd.gplite import _device_gp_with_noise

    dgp = _device_gp_with_noise(eng, gp2)
    # the state travels through the mirror's one-entry cache; the device GP of gp2 is another handle of the same GP
    Xs = c["LB"] + (c["UB"] - c["LB"]) * rng.random((40, D))
    base = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": False, "TolGPVar": 1e-4, "gplengthscale": gl}
    st_dev = dict(base, ActiveImportanceSampling={"Xa": d["Xa"], "lnw": d["lnw"], "fs2a": d["fs2a"], "_device": (dgp, d["state"])})
    st_up = dict(base, ActiveImportanceSampling={"Xa": d["Xa"], "lnw": d["lnw"], "fs2a": d["fs2a"]})
    vp = Q.build_case("D3")["vp"]
    a = va.acqwrapper_vbmc(Xs, vp, gp2, st_dev, False, "acqimiqr_vbmc", nargout=3)
    b = va.acqwrapper_vbmc(Xs, vp, gp2, st_up, False, "acqimiqr_vbmc", nargout=3)
    assert st_dev["ActiveImportanceSampling"]["_device"][1] is d["state"]
    for u, v in zip(a, b):
        assert np.all(np.isfinite(u)) and np.array_equal(u, v)
    # vbmc_acq_search_iqr accepts the returned state
    x0 = 0.5 * (c["LB"] + c["UB"])
    r = va.acq_search(x0, 0.1 * (c["UB"] - c["LB"]), c["LB"], c["UB"], vp, gp2, st_dev, "acqimiqr_vbmc", TolX=0.0, TolFun=0.0, TolHistFun=0.0,
                      MaxIter=3, seed=1)
    assert r["generations"] == 3 and np.isfinite(r["fbest"])
    assert st_dev["ActiveImportanceSampling"]["_device"][1] is d["state"]


def test_errors_leave_the_context_usable(va):
    c, _ = I.run_case("A")

    def ok():
        r = device_run(va, c, spec=3)
        assert r["funccount"] > 0 and np.all(np.isfinite(r["lnw"]))

    def invalid(match, **kw):
        with pytest.raises(va.VbmcHipError, match=match) as e:
            device_run(va, c, **kw)
        assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1
        ok()

    ok()
    S, W, D = c["x0"].shape
    invalid("W = 5", x0=c["x0"][:, :5], uniforms=None)
    invalid("W = 2", x0=c["x0"][:, :2], uniforms=None)
    invalid("LB < UB", LB=c["UB"])
    x0 = c["x0"].copy()
    x0[1, 2, 0] = c["UB"][0] + 1.0
    invalid("outside the box", x0=x0)
    invalid("Nm = 257", Nm=257, uniforms=None)
    invalid("spec = 5", spec=5)
    invalid("uniform block exhausted", uniforms=c["U"][:, :, :, :2])
    U0 = c["U"].copy()
    U0[2, 1, 1, 0] = 0.0
    invalid("strictly inside", uniforms=U0)
    with pytest.raises(ValueError, match="hyper-samples"):                      # x0 laid out for another S: refused before the call
        device_run(va, c, x0=c["x0"][:1], uniforms=None)
    ok()
    # a start with -Inf density: a hyper-sample whose mean sends the prediction to -Inf at the walkers
    gpi = dict(c["gp"], post=[dict(p) for p in c["gp"]["post"]])
    gpi["post"][0] = dict(gpi["post"][0], alpha=np.full_like(gpi["post"][0]["alpha"], -1e308))
    invalid("zero density", gp=gpi)
    # a GP handle without vbmc_gp_set_noise
    import ctypes as C

    from vbmc_amd._lib import IsSampleArgs, new_args
    from vbmc_amd.acq import f64, ptr

    eng = va.default_engine()
    bare = eng.device_gp(dict(c["gp"], post=list(c["gp"]["post"])), need_L=True)      # a handle of its own, its noise model not set
    a = new_args(IsSampleArgs)
    a.W, a.D, a.S, a.Nm, a.thin, a.burnin = W, D, S, c["Nm"], 1, -1
    keep = (f64(np.transpose(c["x0"], (1, 2, 0))), f64(c["LB"]), f64(c["UB"]))
    a.x0, a.LB, a.UB = ptr(keep[0]), ptr(keep[1]), ptr(keep[2])
    st = eng.ctx.lib.vbmc_acq_is_sample(eng.ctx.h, bare.h, C.byref(a))
    assert st == 1 and b"vbmc_gp_set_noise" in eng.ctx.lib.vbmc_last_error(eng.ctx.h)
    a.D = D + 1                                                                  # the library checks the layout itself, too
    st = eng.ctx.lib.vbmc_acq_is_sample(eng.ctx.h, bare.h, C.byref(a))
    assert st == 1 and b"laid out" in eng.ctx.lib.vbmc_last_error(eng.ctx.h)
    ok()


def test_large_n_is_unsupported(va):
    """N = 1264 is the prediction's slab form: the status only (nothing of the sampler is launched)."""
    from tests import _quad_ref as Q

    gp, _ = Q.mixed_gp(1, 4, 1264, 1, 4)
    X = gp["X"]
    W = 10
    x0 = X[:W][None, :, :]
    with pytest.raises(va.VbmcUnsupported):
        from vbmc_amd.acq import importance_sample_device

        importance_sample_device(gp, x0, np.min(X, axis=0) - 1.0, np.max(X, axis=0) + 1.0, 4, seed=1)


def test_end_to_end_through_the_mirror(va):
    from tests import _acqsearch_iqr_ref as Q
    from tests._quad_ref import mixed_gp

    D, N, S = 3, 60, 3
    gp, _ = mixed_gp(2, D, N, S, 4)
    rng = np.random.default_rng(11)
    X = gp["X"]
    vp = Q.build_case("D3")["vp"]
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    gp = dict(gp, X_rescaled=X / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    opts = {"ActiveImportanceSamplingMCMCSamples": 24, "ActiveImportanceSamplingVPSamples": 30, "ActiveImportanceSamplingBoxSamples": 30}
    ais = va.activeimportancesampling_vbmc(vp, gp, "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(3), device=True)
    assert ais["Xa"].shape == (24, D, S) and ais["lnw"].shape == (S, 24) and ais["fs2a"].shape == (24, S)
    assert "_device" in ais and ais["funccount"] > 0
    # lnw + logp = fmu: the chain's own logp, against an independent oracle prediction of fmu at the returned points; the chain's logp
    # is itself the oracle's target there
    tgt = I.oracle_target(gp)
    assert ais["logp"].shape == (S, 24)
    for s in range(S):
        fm = np.asarray(R.gplite_pred(gp, ais["Xa"][:, :, s], None, None, True)[2]).reshape(24, -1)[:, s]
        lp = ais["logp"][s]
        assert float(np.max(np.abs(lp - tgt(ais["Xa"][:, :, s], s)) / np.maximum(1.0, np.abs(lp)))) < 1e-9
        err = float(np.max(np.abs(ais["lnw"][s] + lp - fm) / np.maximum(1.0, np.abs(fm))))
        print("end to end, hyper-sample %d: |lnw + logp - fmu| %.2e" % (s, err))
        assert err < 1e-9
    from vbmc_amd.acq import _importance_state
    from vbmc_amd.gplite import _device_gp_with_noise

    eng = va.default_engine()
    carried = ais["_device"][1]
    st = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": False, "TolGPVar": 1e-4, "gplengthscale": gl, "ActiveImportanceSampling": ais}
    Xs = X[:20] + 0.1 * rng.standard_normal((20, D))
    acq = va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqimiqr_vbmc")
    assert np.all(np.isfinite(acq))
    assert _importance_state(eng, _device_gp_with_noise(eng, gp), ais) is carried
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    r = va.acq_search(Xs[int(np.argmin(acq))], 0.1 * diam, np.min(X, axis=0) - 0.5 * diam, np.max(X, axis=0) + 0.5 * diam, vp, gp, st, "acqimiqr_vbmc",
                      TolX=0.0, TolFun=0.0, TolHistFun=0.0, MaxIter=4, seed=2)
    assert r["generations"] == 4 and np.isfinite(r["fbest"])
    assert ais["_device"][1] is carried

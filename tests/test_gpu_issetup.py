"""GPU: the one-call set-up of the IMIQR importance sampler (vbmc_acq_is_setup) in parity mode against the NumPy restatement
tests/_issetup_ref.py fed the oracle's gplite_pred, on the cases of that file.

Tolerances.  Xa1, rect_delta, LB, UB, idx0 and x0: identical -- the points are formed from individually rounded operations, and every
resampling draw is guarded by the margin tests/test_issetup_restatement.py asserts for this very table (1e-9 of the total weight, seven
orders above the rounding of a cumulative sum).  lnw1 and fs2a1: 1e-9 relative (fs2a1 on the scale max(1, sf2)), the prediction's
tolerance of tests/test_gpu_issample.py.  The proposal's log density alone, lpdf1 (= fmu - lnw1): LPDF_TOL, ten times the largest
deviation from the oracle measured over these cases (3.6e-15 absolute) and no looser than 1e-10."""
import numpy as np
import pytest

from tests import _issetup_ref as T

pytestmark = pytest.mark.gpu
LPDF_TOL = 3.6e-14         # measured: 3.553e-15 (case D; A 8.9e-16, B 1.8e-15, C 4.4e-16, P 8.9e-16)
STEP1 = ("Xa1", "lnw1", "fs2a1", "lpdf1", "rect_delta", "LB", "UB")
STEP2 = ("Xa", "lnw", "fs2a", "logp")


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def device_run(c, **kw):
    from vbmc_amd.acq import importance_setup_device

    args = dict(block=c["B"], uniforms=c["U"], spec=1)
    args.update(kw)
    gp, vp = args.pop("gp", c["gp"]), args.pop("vp", c["vp"])
    Nvp, Nbox, Nm = args.pop("Nvp", c["Nvp"]), args.pop("Nbox", c["Nbox"]), args.pop("Nm", c["Nm"])
    return importance_setup_device(vp, gp, Nvp, Nbox, Nm, **args)


def same_bits(a, b, what, keys=STEP1 + ("x0", "idx0", "bad") + STEP2):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert (a["n_bad"], a["funccount"]) == (b["n_bad"], b["funccount"]), what


def with_noise(c):
    """the case's GP with what the IQR acquisition functions read beside it, and test points"""
    gp, D, N = c["gp"], c["D"], c["N"]
    rng = np.random.default_rng(5)
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    gp2 = dict(gp, X_rescaled=gp["X"] / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    Xs = gp["X"][:20] + 0.1 * rng.standard_normal((20, D))
    base = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": False, "TolGPVar": 1e-4, "gplengthscale": gl}
    return gp2, Xs, base


def state_equals_upload(va, c, arrays, state):
    """acqimiqr_vbmc through vbmc_acq_iqr_eval: the returned state against vbmc_acq_is_create on the downloaded arrays"""
    from vbmc_amd.gplite import _device_gp_with_noise

    gp2, Xs, base = with_noise(c)
    dgp = _device_gp_with_noise(va.default_engine(), gp2)
    st_dev = dict(base, ActiveImportanceSampling=dict(arrays, _device=(dgp, state)))
    st_up = dict(base, ActiveImportanceSampling=dict(arrays))
    a = va.acqwrapper_vbmc(Xs, c["vp"], gp2, st_dev, False, "acqimiqr_vbmc", nargout=3)
    b = va.acqwrapper_vbmc(Xs, c["vp"], gp2, st_up, False, "acqimiqr_vbmc", nargout=3)
    assert st_dev["ActiveImportanceSampling"]["_device"][1] is state
    for u, v in zip(a, b):
        assert np.all(np.isfinite(u)) and np.array_equal(u, v)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "P"])
def test_step_one_and_the_resampling_against_the_restatement(va, name):
    c, ref = T.run_case(name)
    assert ref["margin"] > T.DRAW_MARGIN
    d = device_run(c)
    S, W, D = c["S"], c["W"], c["D"]
    for k in ("Xa1", "rect_delta", "LB", "UB"):
        assert np.array_equal(d[k], ref[k]), k
    for k in STEP1 + STEP2 + ("x0",):
        assert not np.any(np.isnan(d[k])), k
    fin = np.isfinite(ref["lnw1"])
    assert np.array_equal(np.isfinite(d["lnw1"]), fin) and np.all(d["lnw1"][~fin] == -np.inf)
    assert np.array_equal(np.isfinite(d["lpdf1"]), np.isfinite(ref["lpdf1"]))
    pf = np.isfinite(ref["lpdf1"])
    sf2 = np.array([np.exp(2 * p["hyp"][D]) for p in c["gp"]["post"]])
    fmu = ref["fmu1"].T
    scale = np.maximum(1.0, np.maximum(np.abs(fmu), np.abs(ref["lpdf1"])[None, :]))
    eW = float(np.max(np.abs(d["lnw1"][fin] - ref["lnw1"][fin]) / scale[fin]))
    eF = float(np.max(np.abs(d["fs2a1"] - ref["fs2a1"]) / np.maximum(1.0, sf2)[None, :]))
    eP = float(np.max(np.abs(d["lpdf1"][pf] - ref["lpdf1"][pf])))
    # the same density with fmu subtracted back out of lnw1: the output lpdf1 is what lnw1 was made of
    eB = float(np.max(np.abs((fmu - d["lnw1"])[fin] - np.broadcast_to(ref["lpdf1"][None, :], fin.shape)[fin]) / scale[fin]))
    print("%s: lnw1 %.2e  fs2a1 %.2e  lpdf1 %.3e (fmu - lnw1: %.2e)  margin %.2e" % (name, eW, eF, eP, eB, ref["margin"]))
    assert eW < 1e-9 and eF < 1e-9 and eB < 1e-9
    assert eP < LPDF_TOL
    assert d["n_bad"] == 0 and not np.any(d["bad"])
    assert np.array_equal(d["idx0"], ref["idx0"])                              # every one of the W S draws
    assert np.array_equal(d["x0"], ref["x0"])
    assert d["Xa"].shape == (c["Nm"], D, S) and np.all(np.isfinite(d["lnw"])) and d["funccount"] > S * W
    assert np.all(d["Xa"] >= d["LB"][None, :, None]) and np.all(d["Xa"] <= d["UB"][None, :, None])
    if name == "P":
        assert np.all(d["lnw1"][:, 0] == -np.inf) and d["lpdf1"][0] == -np.inf and not np.any(d["idx0"] == 0)


@pytest.mark.parametrize("name", ["A", "D"])
def test_device_generator_replays_through_its_dumps(va, name):
    from vbmc_amd.acq import importance_sample_rng_dump, importance_setup_rng_dump

    c, _ = T.run_case(name)
    seed = 20240611
    a = device_run(c, block=None, uniforms=None, seed=seed, spec=3)
    B = importance_setup_rng_dump(seed, c["D"], c["S"], c["W"], c["Nvp"], c["Nbox"])
    U = importance_sample_rng_dump(seed, c["S"], c["W"] // 2, c["U"].shape[3] + 8)
    b = device_run(c, block=B, uniforms=U, seed=0, spec=3)
    same_bits(a, b, "replay")
    assert a["performed"] == b["performed"] and a["rounds"] == b["rounds"] and a["n_bad"] == 0
    e = device_run(c, block=B, uniforms=None, seed=seed, spec=2)               # Step 2 from the seed beside a supplied Step 1 block
    same_bits(a, e, "block + seed")


@pytest.mark.parametrize("name", ["A", "C"])
def test_chaining_equals_the_two_calls(va, name):
    from vbmc_amd.acq import importance_sample_device

    c, _ = T.run_case(name)
    d = device_run(c, spec=3)
    r = importance_sample_device(c["gp"], d["x0"], d["LB"], d["UB"], c["Nm"], uniforms=c["U"], spec=2)
    for k in STEP2:
        assert np.array_equal(d[k], r[k]), k
    assert d["funccount"] == r["funccount"]
    s = device_run(c, block=c["B"], uniforms=None, seed=99, spec=3)             # the same with the Step-2 seed
    r = importance_sample_device(c["gp"], s["x0"], s["LB"], s["UB"], c["Nm"], seed=99)
    for k in STEP2:
        assert np.array_equal(s[k], r[k]), k
    state_equals_upload(va, c, {"Xa": d["Xa"], "lnw": d["lnw"], "fs2a": d["fs2a"]}, d["state"])


def test_a_start_of_zero_density_comes_back_to_the_caller(va):
    from tests._issample_ref import oracle_target
    from vbmc_amd.acq import importance_sample_device

    c, ref = T.run_case("Z")
    S, W = c["S"], c["W"]
    lp = oracle_target(c["gp"])
    with np.errstate(all="ignore"):
        expect = ~np.isfinite(np.stack([lp(ref["x0"][s], s) for s in range(S)])).T          # W x S
    assert int(np.sum(expect)) == 1 and expect[5, 1]
    d = device_run(c, spec=3)
    assert d["n_bad"] == 1 and np.array_equal(d["bad"], expect)
    assert np.array_equal(d["idx0"], ref["idx0"]) and np.array_equal(d["x0"], ref["x0"]) and np.array_equal(d["Xa1"], ref["Xa1"])
    assert "Xa" not in d and d["state"] is None and d["funccount"] == S * W and d["rounds"] == 0      # Step 2 has not run
    x0 = d["x0"].copy()
    x0[1, 5] = x0[1, 0]                                                         # the caller's patch: any start of finite density
    r = importance_sample_device(c["gp"], x0, d["LB"], d["UB"], c["Nm"], uniforms=c["U"])
    assert np.all(np.isfinite(r["lnw"]))


def test_step_one_alone(va):
    c, ref = T.run_case("A")
    full = device_run(c)
    n1 = (c["D"] + 1) * c["Na1"]
    d = device_run(c, Nm=0, block=c["B"][:n1], uniforms=None)
    for k in STEP1:
        assert np.array_equal(d[k], full[k]), k
    assert "x0" not in d and "Xa" not in d and d["funccount"] == 0 and d["state"] is not None
    state_equals_upload(va, c, {"Xa": d["Xa1"], "lnw": d["lnw1"], "fs2a": d["fs2a1"]}, d["state"])


def test_errors_leave_the_context_usable(va):
    import ctypes as C

    from vbmc_amd._lib import IsSetupArgs, new_args
    from vbmc_amd.acq import f64, ptr

    c, _ = T.run_case("A")
    D, S, W, K = c["D"], c["S"], c["W"], c["K"]

    def ok():
        r = device_run(c, spec=3)
        assert r["n_bad"] == 0 and r["funccount"] > 0 and np.all(np.isfinite(r["lnw"]))

    def refused(match, unsupported=False, **kw):
        with pytest.raises(va.VbmcHipError, match=match) as e:
            device_run(c, **kw)
        assert isinstance(e.value, va.VbmcUnsupported) == unsupported and (unsupported or e.value.status == 1)
        ok()

    ok()
    free = dict(block=None, uniforms=None, seed=3)
    refused("Nvp \\+ Nbox = 0", Nvp=0, Nbox=0, **free)
    refused("Nvp \\+ Nbox = 257", Nvp=200, Nbox=57, **free)
    refused("non-negative", Nvp=-1, Nbox=20, **free)
    big = {"D": D, "K": 513, "mu": np.zeros((D, 513)), "sigma": np.ones(513), "lambda": np.ones(D), "w": np.full(513, 1.0 / 513)}
    refused("K = 513", unsupported=True, vp=big, **free)
    for key, val in (("mu", np.nan), ("sigma", 0.0), ("lambda", np.inf), ("w", -0.1)):
        vp = dict(c["vp"], **{key: np.array(c["vp"][key], dtype=np.float64, copy=True)})
        vp[key].reshape(-1)[0] = val
        refused("variational posterior must be finite", vp=vp, **free)
    for j, val in ((0, 0.0), ((D + 1) * c["Nvp"] + 1, 1.0), (1, np.inf), (c["B"].size - 1, 1.5)):
        B = c["B"].copy()
        B[j] = val
        refused("block value %d" % j, block=B)
    refused("W = 5", W=5, **free)
    refused("Nm = 257", Nm=257, **free)
    refused("spec = 5", spec=5)
    refused("uniform block exhausted", uniforms=c["U"][:, :, :, :2])
    U0 = c["U"].copy()
    U0[2, 1, 1, 0] = 0.0
    refused("strictly inside", uniforms=U0)
    # a GP handle without vbmc_gp_set_noise, and a layout that is not the GP's
    eng = va.default_engine()
    bare = eng.device_gp(dict(c["gp"], post=list(c["gp"]["post"])), need_L=True)
    a = new_args(IsSetupArgs)
    a.D, a.S, a.K, a.Nvp, a.Nbox, a.W, a.Nm, a.thin, a.burnin = D, S, K, c["Nvp"], c["Nbox"], W, c["Nm"], 1, -1
    keep = [f64(np.asarray(c["vp"][k], dtype=np.float64)) for k in ("mu", "sigma", "lambda", "w")]
    a.vp_mu, a.vp_sigma, a.vp_lambda, a.vp_w = (ptr(k) for k in keep)
    st = eng.ctx.lib.vbmc_acq_is_setup(eng.ctx.h, bare.h, C.byref(a))
    assert st == 1 and b"vbmc_gp_set_noise" in eng.ctx.lib.vbmc_last_error(eng.ctx.h)
    a.D = D + 1
    st = eng.ctx.lib.vbmc_acq_is_setup(eng.ctx.h, bare.h, C.byref(a))
    assert st == 1 and b"laid out" in eng.ctx.lib.vbmc_last_error(eng.ctx.h)
    a.D, a.struct_size = D, 8
    assert eng.ctx.lib.vbmc_acq_is_setup(eng.ctx.h, bare.h, C.byref(a)) == 1
    ok()


def test_large_n_is_unsupported(va):
    """N = 1264 is the prediction's slab form: the status only, as vbmc_acq_is_sample answers it"""
    from tests import _quad_ref as Q
    from vbmc_amd.acq import importance_setup_device

    gp, _ = Q.mixed_gp(1, 4, 1264, 1, 4)
    vp = {"D": 4, "K": 2, "mu": gp["X"][:2].T.copy(), "sigma": np.full(2, 0.3), "lambda": np.ones(4), "w": np.full(2, 0.5)}
    with pytest.raises(va.VbmcUnsupported):
        importance_setup_device(vp, gp, 10, 10, 4, seed=1)


def test_the_mirror_takes_the_one_call(va, monkeypatch):
    """activeimportancesampling_vbmc(device=True): one call where it applies, the host patch and vbmc_acq_is_sample behind a bad start,
    the path without the one call behind 'unsupported'"""
    from vbmc_amd import acq

    c, _ = T.run_case("A")
    opts = {"ActiveImportanceSamplingMCMCSamples": c["Nm"], "ActiveImportanceSamplingVPSamples": c["Nvp"], "ActiveImportanceSamplingBoxSamples": c["Nbox"]}
    calls = []
    real_setup, real_sample = acq.importance_setup_device, acq.importance_sample_device
    monkeypatch.setattr(acq, "importance_setup_device", lambda *a, **k: (calls.append("setup"), real_setup(*a, **k))[1])
    monkeypatch.setattr(acq, "importance_sample_device", lambda *a, **k: (calls.append("sample"), real_sample(*a, **k))[1])
    ais = va.activeimportancesampling_vbmc(c["vp"], c["gp"], "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(3), device=True, one_call=True)
    assert calls == ["setup"] and ais["Xa"].shape == (c["Nm"], c["D"], c["S"]) and "_device" in ais and np.all(np.isfinite(ais["lnw"]))
    direct = real_setup(c["vp"], c["gp"], c["Nvp"], c["Nbox"], c["Nm"], seed=int(np.random.default_rng(3).integers(0, 2 ** 63)))
    assert np.array_equal(ais["Xa"], direct["Xa"]) and np.array_equal(ais["lnw"], direct["lnw"])
    del calls[:]

    def flagged(*a, **k):                                                      # a start reported bad: the host patch, then vbmc_acq_is_sample
        r = real_setup(*a, **k)
        r["n_bad"] = 1
        r["bad"][2, 1] = True
        for key in STEP2:
            del r[key]
        return r

    monkeypatch.setattr(acq, "importance_setup_device", lambda *a, **k: (calls.append("setup"), flagged(*a, **k))[1])
    ais = va.activeimportancesampling_vbmc(c["vp"], c["gp"], "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(3), device=True, one_call=True)
    assert calls == ["setup", "sample"] and np.all(np.isfinite(ais["lnw"])) and "_device" in ais
    del calls[:]

    def unsupported(*a, **k):
        calls.append("setup")
        raise va.VbmcUnsupported(2, "not accelerated")

    monkeypatch.setattr(acq, "importance_setup_device", unsupported)
    ais = va.activeimportancesampling_vbmc(c["vp"], c["gp"], "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(3), device=True, one_call=True)
    assert calls == ["setup", "sample"] and ais["Xa"].shape == (c["Nm"], c["D"], c["S"])
    del calls[:]
    va.activeimportancesampling_vbmc(c["vp"], c["gp"], "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(3), device=True, one_call=False)
    assert calls == ["sample"]

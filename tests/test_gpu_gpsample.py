"""GPU: the surrogate sampler on the device (vbmc_gp_surrogate_sample, gplite.gplite_sample_device / gplite_sample,
vptools.gpsample_vbmc) against the NumPy restatement tests/_gpsample_ref.py, given the same uniforms (parity mode), on the cases of
that file.

Tolerances.  Xt: 1e-10 of the box; logp: 1e-9 of max(1, |logp|) -- the figures and the reasoning of tests/test_gpu_issample.py (the
decisions are identical: tests/test_gpsample_restatement.py asserts the 1e-6 margin for this very table; the prediction's tolerance
against the oracle is 1e-9).  sn2_avg: 1e-10 relative (a mean of identical terms, summed in another order).  Original-space samples:
XORIG_TOL of tests/test_gpu_vptools.py, against warpvars 'inv' of the device's own records."""
import ctypes as C

import numpy as np
import pytest

from tests import _gpsample_ref as G
from tests.test_gpu_vptools import XORIG_TOL

pytestmark = pytest.mark.gpu
KEYS = ("X", "Xt", "logp")


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def device_run(va, c, **kw):
    from vbmc_amd.gplite import gplite_sample_device

    args = dict(x0=c["x0"], E=c["E"], thin=c["thin"], beta=c["beta"], VarThresh=c["VarThresh"], uniforms=c["U"], spec=1)
    args.update(kw)
    gp = args.pop("gp", c["gp"])
    LB, UB = args.pop("LB", c["LB"]), args.pop("UB", c["UB"])
    Ns = args.pop("Ns", c["Ns"])
    return gplite_sample_device(gp, Ns, LB, UB, **args)


def same_bits(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["funccount"] == b["funccount"], what


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_parity_with_the_restatement(va, name):
    c, ref = G.run_case(name)
    assert ref["margin"] > G.MARGIN
    d = device_run(va, c)
    span = (c["UB"] - c["LB"])[None, :, None]
    eX = float(np.max(np.abs(d["Xt"] - ref["Xa"]) / span))
    eL = float(np.max(np.abs(d["logp"] - ref["logp"]) / np.maximum(1.0, np.abs(ref["logp"]))))
    print("%s: Xt %.2e  logp %.2e  funccount %d / %d  rounds %d" % (name, eX, eL, d["funccount"], ref["funccount"], d["rounds"]))
    assert d["funccount"] == ref["funccount"]
    assert eX < 1e-10
    assert eL < 1e-9
    assert d["Xt"].shape == (c["Nm"], c["D"], c["E"]) and d["X"].shape == (c["Ns"], c["D"]) and d["logp"].shape == (c["E"], c["Nm"])
    assert np.array_equal(d["X"], G.interleave(d["Xt"], c["Ns"]))                 # origflag = 0: the interleaved records, bit for bit
    assert np.array_equal(d["x0"], c["x0"])                                       # a start inside the box comes back as it went in
    assert np.all(d["Xt"] >= c["LB"][None, :, None]) and np.all(d["Xt"] <= c["UB"][None, :, None])
    assert d["VarThresh"] == c["VarThresh"] and d["sn2_avg"] == 0.0
    if name == "E":
        assert ref["outside"] > 0
    if name == "G":                                                               # one more training input: refused, the next call unaffected
        from oracle import vbmc_ref as R
        from tests._cases import synth_problem

        D = c["D"]
        p = synth_problem(1, D, 1137, 3, 1, meanfun=1, noisy=False)
        big = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=1, noisefun=p["noisefun"], s2=p["s2"])
        with pytest.raises(va.VbmcUnsupported, match="resident"):
            device_run(va, c, gp=big, E=1, x0=c["x0"], uniforms=None, seed=1)
        same_bits(d, device_run(va, c), "after the refusal")


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_spec_and_chunk_change_no_bit(va, name):
    c, _ = G.run_case(name)
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
    from vbmc_amd.gplite import gp_surrogate_sample_rng_dump

    c, _ = G.run_case("B")
    a = device_run(va, c, uniforms=None, seed=20240607, spec=3)
    U = gp_surrogate_sample_rng_dump(20240607, c["E"], c["H"], 4 * c["M"])
    b = device_run(va, c, uniforms=U, spec=3)
    same_bits(a, b, "replay")
    assert a["performed"] == b["performed"] and a["rounds"] == b["rounds"]


@pytest.mark.parametrize("name", sorted(G.VP_CASES))
def test_vp_driven_form(va, name):
    from tests import _vptools_ref as T
    from vbmc_amd import vptools as V
    from vbmc_amd.gplite import gplite_sample_device

    c = G.build_vp_case(name)
    vp, gp, nz, D = c["vp"], c["gp"], c["noise"], c["D"]
    E, W, Ns, seed = 2, 2 * (D + 1), 21, G.VP_SEED
    counts = (G.NNN, 20000) if name == "B" else (G.NNN,)
    for Nnn in counts:
        d = gplite_sample_device(gp, Ns, c["LB"], c["UB"], vp=vp, E=E, noise=dict(nz, Nnn=Nnn), origflag=True, seed=seed, spec=3)
        # the start: the posterior's own unbalanced transformed-space draws, draw w + W e the walker w of ensemble e, clipped
        Y0 = V.vbmc_rnd(vp, W * E, False, False, seed=seed, nargout=1)
        want = np.minimum(np.maximum(Y0, c["LB"]), c["UB"]).reshape(E, W, D)
        assert np.array_equal(d["x0"], want)
        assert np.any(want != Y0.reshape(E, W, D))                                # the clip acted
        # the noise estimate
        Yn = V.vbmc_rnd(vp, Nnn, False, False, seed=seed + 1, nargout=1)
        pos, avg, _, gap = G.noise_estimate(Yn, nz["gplengthscale"], nz["X_rescaled"], nz["sn2new"])
        assert gap > G.GAP
        assert np.array_equal(d["sn2_nn"], nz["sn2new"][pos])                     # distinct values: the nearest indices are identical
        err = abs(d["sn2_avg"] - avg) / abs(avg)
        print("%s Nnn %d: sn2_avg %.6f  rel err %.2e  VarThresh %.6f" % (name, Nnn, d["sn2_avg"], err, d["VarThresh"]))
        assert err < 1e-10
        assert d["VarThresh"] == max(1.0, d["sn2_avg"])
        # the way back: warpvars 'inv' of the device's own records
        Xi = T.warp(G.interleave(d["Xt"], Ns), "i", vp["trinfo"])
        eo = float(np.max(np.abs(d["X"] - Xi) / np.maximum(1.0, np.abs(Xi))))
        print("%s: X orig %.3e" % (name, eo))
        assert eo <= XORIG_TOL
        lo, hi = T.clamp_ends(vp["trinfo"])
        assert np.all(d["X"] >= lo) and np.all(d["X"] <= hi)
        t = gplite_sample_device(gp, Ns, c["LB"], c["UB"], vp=vp, E=E, noise=dict(nz, Nnn=Nnn), origflag=False, seed=seed, spec=3)
        assert np.array_equal(t["Xt"], d["Xt"]) and np.array_equal(t["X"], G.interleave(t["Xt"], Ns))
    # the threshold the estimate set is the one the chain ran on: the same call with it as an argument and the start handed over
    h = gplite_sample_device(gp, Ns, c["LB"], c["UB"], x0=d["x0"], E=E, VarThresh=d["VarThresh"], seed=seed, spec=3)
    assert np.array_equal(h["Xt"], d["Xt"]) and np.array_equal(h["logp"], d["logp"])


def test_errors_leave_the_context_usable(va):
    from vbmc_amd import _lib
    from vbmc_amd.acq import f64, ptr
    from vbmc_amd.gplite import _device_gp_with_noise, gplite_sample_device

    c, _ = G.run_case("A")
    first = device_run(va, c, spec=3)

    def ok():
        same_bits(first, device_run(va, c, spec=3), "after an error")

    def invalid(match, **kw):
        with pytest.raises(va.VbmcHipError, match=match) as e:
            device_run(va, c, **kw)
        assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1
        ok()

    def unsupported(match, **kw):
        with pytest.raises(va.VbmcUnsupported, match=match):
            device_run(va, c, **kw)
        ok()

    E, W, D = c["x0"].shape
    invalid("W = 5", x0=c["x0"][:, :5], uniforms=None)
    invalid("W = 2", x0=c["x0"][:, :2], uniforms=None)
    invalid("W = 8", x0=np.concatenate([c["x0"], c["x0"][:, :2]], axis=1), uniforms=None)      # beyond 2 (D + 1)
    invalid("LB < UB", LB=c["UB"])
    invalid("thin", thin=0)
    invalid("spec = 5", spec=5)
    invalid("max_steps", max_steps=21)
    invalid("Ns = 0", Ns=0)
    invalid("E = 0", E=0, x0=None, uniforms=None, vp=G.build_vp_case("C")["vp"])
    invalid("E = 65", E=65, x0=None, uniforms=None, vp=G.build_vp_case("C")["vp"])
    invalid("burnin", burnin=-2)
    invalid("uniform block exhausted", uniforms=c["U"][:, :, :, :2])
    U0 = c["U"].copy()
    U0[2, 1, 0, 0] = 0.0
    invalid("strictly inside", uniforms=U0)
    invalid("posterior is needed", x0=None, uniforms=None)                       # no x0, no vp
    invalid("posterior is needed", origflag=True)
    invalid("posterior is needed", noise={"X_rescaled": c["gp"]["X"], "gplengthscale": np.ones(D), "sn2new": np.ones(c["N"])})
    # a start with -Inf density: a hyper-sample whose mean sends the prediction to -Inf at the walkers
    gpi = dict(c["gp"], post=[dict(p) for p in c["gp"]["post"]])
    gpi["post"][0] = dict(gpi["post"][0], alpha=np.full_like(gpi["post"][0]["alpha"], -1e308))
    invalid("zero density", gp=gpi)
    # E Nm D doubles above 1 GiB (refused before anything is allocated), a transform the vp tools refuse
    unsupported("1 GiB", Ns=2 ** 27, outputs=())
    vpc = G.build_vp_case("C")
    bad = dict(vpc["vp"], trinfo=dict(vpc["vp"]["trinfo"], type=np.array([3, 5, 3])))
    with pytest.raises(va.VbmcUnsupported, match="transform type"):
        gplite_sample_device(vpc["gp"], 8, vpc["LB"], vpc["UB"], vp=bad, seed=1)
    ok()
    # the library checks the layout and the noise estimate's arrays itself
    eng = va.default_engine()
    dgp = _device_gp_with_noise(eng, c["gp"])
    a = _lib.new_args(_lib.GsArgs)
    a.D, a.S, a.E, a.Ns, a.thin, a.burnin, a.VarThresh = D, 1, 1, 8, 1, -1, np.inf
    keep = (f64(np.transpose(c["x0"], (1, 2, 0))), f64(c["LB"]), f64(c["UB"]), f64(np.ones(c["N"])))
    a.x0, a.LB, a.UB, a.W = ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), W
    lib, h = eng.ctx.lib, eng.ctx.h
    assert lib.vbmc_gp_surrogate_sample(h, dgp.h, None, C.byref(a)) == 0
    a.D = D + 1
    assert lib.vbmc_gp_surrogate_sample(h, dgp.h, None, C.byref(a)) == 1 and b"laid out" in lib.vbmc_last_error(h)
    a.D = D
    a.sn2new = ptr(keep[3])
    assert lib.vbmc_gp_surrogate_sample(h, dgp.h, None, C.byref(a)) == 1 and b"X_rescaled" in lib.vbmc_last_error(h)
    a.sn2new = None
    a.struct_size += 8
    assert lib.vbmc_gp_surrogate_sample(h, dgp.h, None, C.byref(a)) == 1 and b"struct_size" in lib.vbmc_last_error(h)
    bare = eng.device_gp(dict(c["gp"], post=list(c["gp"]["post"])), need_L=True)  # a handle of its own, its noise model not set
    a.struct_size -= 8
    assert lib.vbmc_gp_surrogate_sample(h, bare.h, None, C.byref(a)) == 1 and b"vbmc_gp_set_noise" in lib.vbmc_last_error(h)
    ok()


def test_gplite_sample_mirror(va):
    """gplite_sample: the reference's argument order, the default box, the HPD start; what is not accelerated is refused"""
    from vbmc_amd.gplite import gplite_sample

    c, _ = G.run_case("C")
    gp, D = c["gp"], c["D"]
    X, r = gplite_sample(gp, 30, None, "parallel", None, 0.5, 2.0, seed=3, nargout=2)
    diam = np.max(gp["X"], axis=0) - np.min(gp["X"], axis=0)
    assert X.shape == (30, D) and np.all(X >= np.min(gp["X"], axis=0) - 10 * diam) and np.all(X <= np.max(gp["X"], axis=0) + 10 * diam)
    assert r["x0"].shape == (1, 2 * (D + 1), D)
    hpd = gp["X"][np.argsort(-gp["y"], kind="stable")[:10]]                       # N_hpd = max(W, round(0.25 N)) = 10 of N = 40
    assert all(any(np.array_equal(w, h) for h in hpd) for w in r["x0"][0])
    assert len({tuple(w) for w in r["x0"][0]}) == 2 * (D + 1)                     # randperm: no walker twice
    X2 = gplite_sample(gp, 30, None, "parallel", None, 0.5, 2.0, seed=3)
    assert np.array_equal(X, X2)
    Xb = gplite_sample(gp, 12, c["x0"][0], "parallel", bounds=np.stack([c["LB"], c["UB"]]), E=1, seed=5)
    assert Xb.shape == (12, D) and np.all(Xb >= c["LB"]) and np.all(Xb <= c["UB"])
    for kw in (dict(method="slicesample"), dict(method=None), dict(logprior=lambda x: 0.0), dict(proppdf=lambda x: 0.0), dict(proprnd=lambda x: x)):
        with pytest.raises(va.VbmcUnsupported):
            gplite_sample(gp, 8, **kw)
    with pytest.raises(va.VbmcUnsupported):                                       # vbmc_rnd(..., 'gp') keeps refusing: a vp carries no gp
        va.vptools.vbmc_rnd(G.build_vp_case("C")["vp"], 5, True, "gp")


def test_gplite_sample_falls_back_beyond_the_resident_range(va):
    """N = 1137: the device call refuses, gplite_sample runs the host-driven sampler over device gplite_pred calls (its own generator:
    no parity; the samples lie in the box and the target at them is finite)"""
    from oracle import vbmc_ref as R
    from tests._cases import synth_problem
    from vbmc_amd.gplite import gplite_sample

    D = 3
    p = synth_problem(1, D, 1137, 3, 1, meanfun=1, noisy=False)
    big = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=1, noisefun=p["noisefun"], s2=p["s2"])
    X, r = gplite_sample(big, 7, None, "parallel", None, 0.0, 1.0, E=2, seed=4, nargout=2)
    assert r is None and X.shape == (7, D) and np.all(np.isfinite(X))
    diam = np.max(big["X"], axis=0) - np.min(big["X"], axis=0)
    assert np.all(X >= np.min(big["X"], axis=0) - 10 * diam) and np.all(X <= np.max(big["X"], axis=0) + 10 * diam)
    assert np.all(np.isfinite(G.log_gpfun(big, 1.0, 0.0)(X, 0)))


def test_end_to_end_gaussian_target(va):
    """gpsample_vbmc on the Gaussian target of tests/test_gpu_system.py: a surrogate whose mean function is the target's log density,
    a posterior somewhere near; the sample mean within the reference's own pass criterion (RMSE < 0.5, test/runtest_vbmc.m:9)."""
    rng = np.random.default_rng(2024)
    D, N, K, Ns = 3, 90, 2, 3000
    mu_t = np.array([0.5, -0.3, 0.2])
    sig_t = np.array([1.0, 0.7, 1.3])
    X = mu_t + 1.4 * sig_t * rng.standard_normal((N, D))
    y = -0.5 * np.sum(((X - mu_t) / sig_t) ** 2, axis=1) - np.sum(np.log(sig_t)) - 0.5 * D * np.log(2 * np.pi)
    # [log ell (D); log sf; log sn; m0; xm (D); log omega (D)]: the negative quadratic mean is the target itself
    m0 = -np.sum(np.log(sig_t)) - 0.5 * D * np.log(2 * np.pi)
    hyp = np.concatenate([np.zeros(D), [np.log(0.1)], [np.log(1e-2)], [m0], mu_t, np.log(sig_t)])
    gp = va.gplite_post(hyp.reshape(-1, 1), X, y, 1, 4)
    idx = rng.permutation(N)[:K]
    vp = va.make_vp(X[idx].T.copy(), np.full(K, 0.5), np.ones(D), eta=np.zeros(K))
    vp["w"] = np.full(K, 1.0 / K)
    Xs, r = va.vptools.gpsample_vbmc(vp, gp, Ns, True, seed=11, nargout=2)
    rmse = float(np.sqrt(np.mean((np.mean(Xs, axis=0) - mu_t) ** 2)))
    sd = np.std(Xs, axis=0)
    print("end to end: mean %s  sd %s  rmse %.3f  rounds %d  performed / funccount %.2f" % (np.mean(Xs, axis=0), sd, rmse, r["rounds"],
                                                                                        r["performed"] / r["funccount"]))
    assert Xs.shape == (Ns, D) and np.all(np.isfinite(Xs))
    assert r["VarThresh"] == 1.0 and r["sn2_avg"] == 0.0                          # a GP without s2: no estimate (gpsample_vbmc.m:34-38)
    assert rmse < 0.5
    assert np.array_equal(Xs, G.interleave(r["Xt"], Ns))                          # no trinfo: the identity
    Xe = va.vptools.gpsample_vbmc(vp, gp, Ns, False, seed=11, E=8)
    rm8 = float(np.sqrt(np.mean((np.mean(Xe, axis=0) - mu_t) ** 2)))
    print("end to end, E = 8: rmse %.3f" % rm8)
    assert rm8 < 0.5

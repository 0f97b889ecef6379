"""GPU: the device-resident search of the IQR acquisition functions (vbmc_acq_search_iqr) against the NumPy restatement
tests/_acqsearch_ref.py::cmaes_chol run over the oracle's acqwrapper_vbmc("acqviqr" | "acqimiqr"), given the same normals (parity mode),
on the cases of tests/_acqsearch_iqr_ref.py.

Tolerances.  Sorted values: 1e-8 (1 + |F|) -- the project's tolerance for the IQR value against the oracle
(tests/test_gpu_acq.py::test_acqviqr_matches_oracle, the acqviqr golden vectors), on the scale of a log-valued function -- with
identical rank orders, guarded by the 1e-6 rank gap tests/test_acqsearch_iqr_restatement.py asserts.  xmean (relative to UB - LB), sigma
and the final C (relative to its largest entry): 1e-9, tests/test_gpu_acqsearch.py's figure -- given identical ranks they are functions
of Z alone."""
import numpy as np
import pytest

from tests import _acqsearch_iqr_ref as I

pytestmark = pytest.mark.gpu
GENS = I.GENS
_CACHE = {}
KEYS_ARR = ("xmin", "xbest", "xmean", "C", "tr_order", "tr_F", "tr_xmean", "tr_sigma")
KEYS_SC = ("fmin", "fbest", "sigma", "evals", "generations", "stop")


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def case_and_ref(name):
    if name not in _CACHE:
        c = I.build_case(name)
        _CACHE[name] = (c, I.run_case(c))
    return _CACHE[name]


def device_run(va, c, **kw):
    args = dict(TolX=0.0, TolFun=0.0, TolHistFun=0.0, MaxIter=GENS, Z=c["Z"], trace=GENS, popsize=c["popsize"])
    args.update(kw)
    st = args.pop("st", c["st"])
    gp = args.pop("gp", c["gp"])
    vp = args.pop("vp", c["vp"])
    acq = args.pop("acq", c["acq"] + "_vbmc")
    return va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], vp, gp, st, acq, **args)


def fresh_state(c):
    """optimState with a copy of ActiveImportanceSampling: no device state cached on it yet."""
    ais = {k: v for k, v in c["st"]["ActiveImportanceSampling"].items() if k != "_device"}
    return dict(c["st"], ActiveImportanceSampling=ais)


def compare_trajectory(c, ref, dev, label):
    tr = ref["trace"]
    assert dev["generations"] == ref["generations"] == GENS and dev["stop"] == ref["stop"] == "MaxIter"
    assert dev["evals"] == ref["evals"] == GENS * c["lam"]
    span = c["UB"] - c["LB"]
    worst = {"F": 0.0, "xmean": 0.0, "sigma": 0.0}
    for g, t in enumerate(tr):
        assert np.array_equal(dev["tr_order"][:, g], t["order"]), (label, g, dev["tr_order"][:, g], t["order"])
        worst["F"] = max(worst["F"], float(np.max(np.abs(dev["tr_F"][:, g] - t["F"]) / (1 + np.abs(t["F"])))))
        worst["xmean"] = max(worst["xmean"], float(np.max(np.abs(dev["tr_xmean"][:, g] - t["xmean"]) / span)))
        worst["sigma"] = max(worst["sigma"], abs(dev["tr_sigma"][g] - t["sigma"]) / t["sigma"])
    eC = float(np.max(np.abs(dev["C"] - ref["C"])) / np.max(np.abs(ref["C"])))
    print("%s: F %.2e  xmean %.2e  sigma %.2e  C %.2e" % (label, worst["F"], worst["xmean"], worst["sigma"], eC))
    assert worst["F"] < 1e-8
    assert worst["xmean"] < 1e-9 and worst["sigma"] < 1e-9 and eC < 1e-9
    assert np.max(np.abs(dev["xmean"] - ref["xmean"]) / span) < 1e-9 and abs(dev["sigma"] - ref["sigma"]) < 1e-9 * ref["sigma"]
    assert np.array_equal(dev["C"], dev["C"].T)
    assert abs(dev["fbest"] - ref["fbest"]) < 1e-8 * (1 + abs(ref["fbest"])) and abs(dev["fmin"] - ref["fmin"]) < 1e-8 * (1 + abs(ref["fmin"]))


@pytest.mark.parametrize("name", sorted(I.iqr_cases()))
def test_trajectory_matches_restatement(va, name):
    c, ref = case_and_ref(name)
    if I.iqr_cases()[name][2] == 3:
        assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False, True]
    compare_trajectory(c, ref, device_run(va, c), name)


def test_state_computed_on_the_device(va):
    """ActiveImportanceSampling = {"Xa"} only: Ctmp and fs2a come from vbmc_acq_is_create; same ranks, same bound."""
    c, ref = case_and_ref("D3")
    st = dict(c["st"], ActiveImportanceSampling={"Xa": c["st"]["ActiveImportanceSampling"]["Xa"]})
    compare_trajectory(c, ref, device_run(va, c, st=st), "D3 device state")


@pytest.mark.parametrize("name", ["D10", "D3", "D5", "face"])
def test_best_value_is_the_sweep_value_at_the_best_point(va, name):
    c, _ = case_and_ref(name)
    r = device_run(va, c, Z=None, seed=11, MaxIter=20, trace=0)
    for x, f in ((r["xbest"], r["fbest"]), (r["xmin"], r["fmin"])):
        assert np.all(x >= c["LB"]) and np.all(x <= c["UB"])
        v = float(va.acqwrapper_vbmc(x[None, :], c["vp"], c["gp"], c["st"], False, c["acq"] + "_vbmc")[0])
        print("%s: sweep %.17g search %.17g" % (name, v, f))
        assert abs(v - f) <= 1e-8 * (1 + abs(v)), (v, f)
    assert r["fbest"] <= r["fmin"]


def same_bits(a, b):
    for k in KEYS_ARR:
        assert np.array_equal(a[k], b[k]), k
    for k in KEYS_SC:
        assert a[k] == b[k], k


def test_device_generator_replays_in_parity_mode(va):
    c, _ = case_and_ref("D10")
    a = device_run(va, c, Z=None, seed=20240607)
    Z = va.acq_search_rng_dump(20240607, c["D"], c["lam"], GENS)
    same_bits(a, device_run(va, c, Z=Z))


def test_results_do_not_depend_on_chunk_or_on_the_run(va):
    c, _ = case_and_ref("D3")
    kw = dict(Z=None, seed=5, MaxIter=0, MaxFunEvals=350, TolX=1e-11 * float(np.max(c["insigma"])), TolFun=1e-12, TolHistFun=1e-13, trace=8)
    runs = [device_run(va, c, chunk=ch, **kw) for ch in (1, 4, 0, 0)]
    for r in runs[1:]:
        same_bits(runs[0], r)
    assert runs[0]["stop"] == "MaxFunEvals" and runs[0]["evals"] == runs[0]["generations"] * c["lam"] == 350


def test_a_value_does_not_depend_on_its_slot_mates(va):
    """popsize 6 and popsize 16 with the same first six columns of normals: generation 0's six points are the same, and so are their
    values to the bit (the sorted trace is compared as a set)."""
    c, _ = case_and_ref("D3")
    D = c["D"]
    rng = np.random.default_rng(77)
    Z6 = rng.standard_normal((D, 6, 2))
    Z16 = rng.standard_normal((D, 16, 2))
    Z16[:, :6, :] = Z6
    a = device_run(va, c, popsize=6, Z=Z6, MaxIter=1, trace=1)
    b = device_run(va, c, popsize=16, Z=Z16, MaxIter=1, trace=1)
    fa, fb = set(a["tr_F"][:, 0].tolist()), set(b["tr_F"][:, 0].tolist())
    assert len(fa) == 6 and len(fb) == 16
    assert fa <= fb, (sorted(fa), sorted(fb))


def test_regulariser_active(va):
    """TolGPVar above a generation-0 point's vtot: the run finishes with finite values and fbest is the device sweep's value at xbest
    within 1e-6 relative (both go through the same fmu / fs2; the bound covers the regulariser's amplification only)."""
    c, _ = case_and_ref("D3")
    X0 = c["x0"][None, :] + 0 * c["insigma"]
    _, _, vtot = va.acqwrapper_vbmc(X0, c["vp"], c["gp"], c["st"], False, "acqviqr_vbmc", nargout=3)
    st = dict(fresh_state(c), TolGPVar=50.0 * float(vtot[0]), VarianceRegularizedAcqFcn=True)
    r = device_run(va, c, st=st, trace=GENS)
    assert r["generations"] == GENS and np.all(np.isfinite(r["tr_F"])) and np.isfinite(r["fbest"])
    v, _, vt = va.acqwrapper_vbmc(r["xbest"][None, :], c["vp"], c["gp"], st, False, "acqviqr_vbmc", nargout=3)
    print("regulariser: vtot(xbest) %.3e TolGPVar %.3e sweep %.17g search %.17g" % (vt[0], st["TolGPVar"], v[0], r["fbest"]))
    assert abs(float(v[0]) - r["fbest"]) <= 1e-6 * abs(float(v[0]))


def test_refusals_leave_the_context_usable(va):
    c, _ = case_and_ref("D3")
    other, _ = case_and_ref("D2")

    def ok():
        r = device_run(va, c, MaxIter=3, trace=0)
        assert r["generations"] == 3 and np.isfinite(r["fbest"])

    ok()
    with pytest.raises(va.VbmcUnsupported):                                   # id 3 through vbmc_acq_search_iqr
        device_run(va, c, acq=3, iqr=True, MaxIter=3)
    ok()
    with pytest.raises(va.VbmcUnsupported, match="vp.delta"):
        device_run(va, c, vp=dict(c["vp"], delta=np.array([0.1, 0.0, 0.0])), MaxIter=3)
    ok()
    # a state created for a different GP (handed over through the mirror's one-entry cache)
    eng = va.default_engine()
    from vbmc_amd.acq import ImportanceState
    from vbmc_amd.gplite import _device_gp_with_noise

    dgp = _device_gp_with_noise(eng, c["gp"])
    foreign = ImportanceState(eng, _device_gp_with_noise(eng, other["gp"]), other["st"]["ActiveImportanceSampling"])
    st = fresh_state(c)
    st["ActiveImportanceSampling"]["_device"] = (dgp, foreign)
    with pytest.raises(va.VbmcHipError, match="belongs to a different GP") as e:
        device_run(va, c, st=st, MaxIter=3)
    assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1
    ok()
    st = dict(c["st"])
    st.pop("gplengthscale")
    with pytest.raises(va.VbmcHipError, match="gplengthscale") as e:
        device_run(va, c, st=st, MaxIter=3)
    assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1
    ok()
    with pytest.raises(va.VbmcHipError, match="popsize") as e:
        device_run(va, c, popsize=17, Z=None, seed=1, MaxIter=3)
    assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1
    ok()
    with pytest.raises(va.VbmcHipError, match="normal block exhausted"):
        device_run(va, c, Z=c["Z"][:, :, :4], MaxIter=10)
    ok()


def test_active_search_with_acqviqr(va):
    c, _ = case_and_ref("D10")
    rng = np.random.default_rng(3)
    Xsearch = c["x0"] + c["insigma"] * rng.standard_normal((200, c["D"]))
    Xsearch = np.minimum(np.maximum(Xsearch, c["LB"]), c["UB"])
    acq = va.acqwrapper_vbmc(Xsearch, c["vp"], c["gp"], c["st"], False, "acqviqr_vbmc")
    x, f, info = va.active_search(Xsearch, c["vp"], c["gp"], c["st"], {"SearchMaxFunEvals": 300}, "acqviqr_vbmc", seed=1)
    assert info["idx"] == int(np.argmin(acq)) and np.array_equal(info["x0"], Xsearch[info["idx"]])
    assert f <= info["fval_old"] and (info["accepted"] == (f < info["fval_old"]))
    assert info["search"]["evals"] <= 300 + c["lam"]

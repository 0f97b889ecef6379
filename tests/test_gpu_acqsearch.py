"""GPU: the device-resident acquisition search (vbmc_acq_search) against the NumPy restatement tests/_acqsearch_ref.py run over the
oracle's acqwrapper_vbmc, given the same normals (parity mode).

Tolerance of the trajectory: 1e-9 relative -- the project's gradient tolerance -- over 20 generations, with identical rank orders:
every sorted value against its own magnitude, |dF| <= 1e-9 |F| (the log-valued acqflog, whose values pass through zero, against 1 + |F|
as tests/test_gpu_acq.py does), xmean relative to UB - LB, sigma, and the final C relative to its largest entry.
The comparison is guarded against ties by the rank-gap precondition tests/test_acqsearch_restatement.py asserts for the same cases.
The shapes are the smallest that reach each edge: D = 2 (lambda = 6), 3, 10 and 32 (lambda = 14, the Cholesky factor across 32 lanes),
N = 17 and 40 (no multiples of 16), S = 1 and S = 3 with the middle hyper-sample on the Lchol = false branch, K = 1 and 2, the four
acquisition functions, the variance regulariser on and off, a start on a face of the box, the two-kernel prediction once, and N = 1264
for the prediction's slab form."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _acqsearch_ref as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENS = 20
_CACHE = {}


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def case_and_ref(name):
    if name not in _CACHE:
        c = A.build_case(name)
        _CACHE[name] = (c, A.run_case(c, GENS))
    return _CACHE[name]


def device_run(va, c, **kw):
    args = dict(TolX=0.0, TolFun=0.0, TolHistFun=0.0, MaxIter=GENS, Z=c["Z"], trace=GENS)
    args.update(kw)
    return va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], c["vp"], c["gp"], c["st"], c["acq"] + "_vbmc", **args)


def f_scale(c, F):
    """What a value's error is measured against: the value itself; 1 + |F| for the log-valued function."""
    return 1 + np.abs(F) if c["acq"] == "acqflog" else np.abs(F)


def compare_trajectory(c, ref, dev, label, gens=GENS):
    tr = ref["trace"]
    assert dev["generations"] == ref["generations"] == gens and dev["stop"] == ref["stop"] == "MaxIter"
    assert dev["evals"] == ref["evals"] == gens * c["lam"]
    span = c["UB"] - c["LB"]
    worst = {"F": 0.0, "xmean": 0.0, "sigma": 0.0}
    for g, t in enumerate(tr):
        assert np.array_equal(dev["tr_order"][:, g], t["order"]), (label, g, dev["tr_order"][:, g], t["order"])
        worst["F"] = max(worst["F"], float(np.max(np.abs(dev["tr_F"][:, g] - t["F"]) / f_scale(c, t["F"]))))
        worst["xmean"] = max(worst["xmean"], float(np.max(np.abs(dev["tr_xmean"][:, g] - t["xmean"]) / span)))
        if np.isfinite(t["sigma"]):
            worst["sigma"] = max(worst["sigma"], abs(dev["tr_sigma"][g] - t["sigma"]) / t["sigma"])
        else:
            assert dev["tr_sigma"][g] == t["sigma"]
    print("%s: F %.2e  xmean %.2e  sigma %.2e" % (label, worst["F"], worst["xmean"], worst["sigma"]))
    assert max(worst.values()) < 1e-9
    assert np.max(np.abs(dev["xmean"] - ref["xmean"]) / span) < 1e-9
    assert np.max(np.abs(dev["xbest"] - ref["xbest"]) / span) < 1e-9 and abs(dev["fbest"] - ref["fbest"]) < 1e-9 * f_scale(c, ref["fbest"])
    assert np.max(np.abs(dev["xmin"] - ref["xmin"]) / span) < 1e-9 and abs(dev["fmin"] - ref["fmin"]) < 1e-9 * f_scale(c, ref["fmin"])
    if np.all(np.isfinite(ref["C"])):
        eC = float(np.max(np.abs(dev["C"] - ref["C"])) / np.max(np.abs(ref["C"])))
        print("%s: C %.2e" % (label, eC))
        assert eC < 1e-9 and abs(dev["sigma"] - ref["sigma"]) < 1e-9 * ref["sigma"]
        assert np.array_equal(dev["C"], dev["C"].T)


@pytest.mark.parametrize("name", sorted(A.search_cases()))
def test_trajectory_matches_restatement(va, name):
    c, ref = case_and_ref(name)
    D, N, S, K, acq, reg, face, _ = A.search_cases()[name]
    if S == 3:
        assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False, True]
    dev = device_run(va, c)
    compare_trajectory(c, ref, dev, name)
    if face:
        assert sum(int(np.sum((t["X"] == c["LB"][:, None]) | (t["X"] == c["UB"][:, None]))) for t in ref["trace"]) > 0


def test_trajectory_two_kernel_prediction():
    """VBMC_PRED_FUSED=0 (read once per process): the same trajectory through k_pred_ks + k_gp_pred."""
    env = dict(os.environ, VBMC_PRED_FUSED="0", PYTHONPATH=ROOT)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import vbmc_amd\n"
            "from tests import test_gpu_acqsearch as T\n"
            "c, ref = T.case_and_ref('D3')\n"
            "T.compare_trajectory(c, ref, T.device_run(vbmc_amd, c), 'D3 two-kernel')\n"
            "print('TRAJECTORY-OK')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "TRAJECTORY-OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_device_generator_replays_in_parity_mode(va):
    c, _ = case_and_ref("D10")
    a = device_run(va, c, Z=None, seed=20240607, MaxIter=12, trace=12)
    Z = va.acq_search_rng_dump(20240607, c["D"], c["lam"], 12)
    assert np.all(np.isfinite(Z)) and abs(float(np.mean(Z))) < 0.2 and 0.8 < float(np.std(Z)) < 1.2
    b = device_run(va, c, Z=Z, MaxIter=12, trace=12)
    for k in ("xmin", "xbest", "xmean", "C", "tr_order", "tr_F", "tr_xmean", "tr_sigma"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("fmin", "fbest", "sigma", "evals", "generations", "stop"):
        assert a[k] == b[k], k


def test_results_do_not_depend_on_chunk(va):
    c, _ = case_and_ref("D3")
    kw = dict(Z=None, seed=5, MaxIter=0, MaxFunEvals=350, TolX=1e-11 * float(np.max(c["insigma"])), TolFun=1e-12, TolHistFun=1e-13, trace=8)
    runs = [device_run(va, c, chunk=ch, **kw) for ch in (1, 4, 0)]
    for r in runs[1:]:
        for k in ("xmin", "xbest", "xmean", "C", "tr_order", "tr_F", "tr_xmean", "tr_sigma"):
            assert np.array_equal(runs[0][k], r[k]), k
        for k in ("fmin", "fbest", "sigma", "evals", "generations", "stop"):
            assert runs[0][k] == r[k], k
    assert runs[0]["stop"] == "MaxFunEvals" and runs[0]["evals"] == runs[0]["generations"] * c["lam"] == 350
    # the launches enqueued behind the end are counted: one chunk read behind, so at most two chunks of them
    assert 0 <= runs[0]["behind"] <= 2 and 0 <= runs[1]["behind"] <= 8 and 0 <= runs[2]["behind"] <= 32


@pytest.mark.parametrize("name", ["D2", "D10", "sn2"])
def test_best_value_is_the_acquisition_at_the_best_point(va, name):
    c, _ = case_and_ref(name)
    r = device_run(va, c, Z=None, seed=11, MaxIter=30, trace=0)
    for x, f in ((r["xbest"], r["fbest"]), (r["xmin"], r["fmin"])):
        assert np.all(x >= c["LB"]) and np.all(x <= c["UB"])
        v = float(va.acqwrapper_vbmc(x[None, :], c["vp"], c["gp"], c["st"], False, c["acq"] + "_vbmc")[0])
        assert abs(v - f) <= 1e-10 * abs(v), (v, f)
    assert r["fbest"] <= r["fmin"]


def test_active_search_never_returns_worse_than_the_sweep(va):
    for name, vpinit in (("D3", True), ("D10", False), ("D2", True)):
        c, _ = case_and_ref(name)
        rng = np.random.default_rng(3)
        Xsearch = c["LB"] + (c["UB"] - c["LB"]) * rng.random((200, c["D"]))
        acq = va.acqwrapper_vbmc(Xsearch, c["vp"], c["gp"], c["st"], False, c["acq"] + "_vbmc")
        x, f, info = va.active_search(Xsearch, c["vp"], c["gp"], c["st"], {"SearchCMAESVPInit": vpinit, "SearchMaxFunEvals": 300},
                                      c["acq"] + "_vbmc", seed=1)
        assert info["idx"] == int(np.argmin(acq)) and np.array_equal(info["x0"], Xsearch[info["idx"]])
        assert f <= info["fval_old"] and (info["accepted"] == (f < info["fval_old"]))
        assert abs(float(va.acqwrapper_vbmc(x[None, :], c["vp"], c["gp"], c["st"], False, c["acq"] + "_vbmc")[0]) - f) <= 1e-10 * abs(f)
        assert info["search"]["evals"] <= 300 + c["lam"]
    with pytest.raises(va.VbmcUnsupported):
        va.active_search(Xsearch, c["vp"], c["gp"], dict(c["st"], integervars=np.array([True, False])), None, "acqf_vbmc")


def test_moments_of_the_variational_posterior(va):
    c, _ = case_and_ref("D3")
    vp = c["vp"]
    X, _ = va.vbmc_rnd(vp, 200000, rng=np.random.default_rng(0))
    m, S = va.vbmc_moments(vp)
    assert np.max(np.abs(m - X.mean(axis=0))) < 0.02 and np.max(np.abs(S - np.cov(X.T))) < 0.03 * np.max(np.abs(S))


def test_refusals_leave_the_context_usable(va):
    c, _ = case_and_ref("D3")
    D = c["D"]

    def run(**kw):
        d = dict(c)
        extra = {k: kw.pop(k) for k in list(kw) if k in ("popsize", "Z", "MaxIter")}
        d.update(kw)
        return va.acq_search(d["x0"], d["insigma"], d["LB"], d["UB"], d["vp"], d["gp"], d["st"], d["acq"] + "_vbmc", TolX=0.0, TolFun=0.0,
                             TolHistFun=0.0, **dict(dict(MaxIter=3, seed=1), **extra))

    def ok():
        r = run()
        assert r["generations"] == 3 and np.isfinite(r["fbest"])

    for kw, exc in [
        (dict(acq="acqviqr"), va.VbmcUnsupported),                                         # an IQR function
        (dict(vp=dict(c["vp"], delta=np.array([0.1, 0.0, 0.0]))), va.VbmcUnsupported),     # vp.delta > 0
    ]:
        with pytest.raises(exc):
            run(**kw)
        ok()
    with pytest.raises(va.VbmcUnsupported):                                                # refused by the mirror, before the library
        va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], c["vp"], c["gp"], c["st"], "acqeig_vbmc", TolX=0, TolFun=0, TolHistFun=0)
    ok()
    # what vbmc_acq_eval refuses, through the C entry: an id outside 0-3 that is no IQR id, and a mixture too large for k_acq's LDS
    for aid in (5, -1):
        with pytest.raises(va.VbmcUnsupported, match="acquisition function id"):
            va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], c["vp"], c["gp"], c["st"], aid, TolX=0, TolFun=0, TolHistFun=0)
        ok()
    Kbig = 1400                                                                            # (2 K D + K) 8 bytes > 64 KiB at D = 3
    rng = np.random.default_rng(0)
    vp_big = dict(c["vp"], K=Kbig, mu=rng.standard_normal((D, Kbig)), sigma=np.full(Kbig, 0.5), w=np.full(Kbig, 1.0 / Kbig))
    for call in (lambda: run(vp=vp_big),
                 lambda: va.acqwrapper_vbmc(c["x0"][None, :], vp_big, c["gp"], c["st"], False, c["acq"] + "_vbmc")):
        with pytest.raises(va.VbmcUnsupported, match="too large"):
            call()
    ok()
    ub_bad = c["UB"].copy(); ub_bad[1] = c["LB"][1]
    lb_inf = c["LB"].copy(); lb_inf[0] = -np.inf
    x_out = c["x0"].copy(); x_out[2] = c["UB"][2] + 1.0
    sg_bad = c["insigma"].copy(); sg_bad[0] = 0.0
    for kw in (dict(UB=ub_bad), dict(LB=lb_inf), dict(x0=x_out), dict(insigma=sg_bad), dict(popsize=17), dict(popsize=1)):
        with pytest.raises(va.VbmcHipError) as e:
            run(**kw)
        assert not isinstance(e.value, va.VbmcUnsupported) and e.value.status == 1, kw
        ok()
    with pytest.raises(va.VbmcHipError, match="normal block exhausted"):
        run(Z=c["Z"][:, :, :4], MaxIter=10)
    ok()


@pytest.mark.parametrize("kind,gens", [("shift", 6), ("indefinite", 1)])
def test_covariance_repair(va, kind, gens):
    """tests/_acqsearch_ref.py::repair_case.  "shift": the initial C is singular, the 1e-14 max diag shift repairs it and the trajectory
    is the restatement's.  "indefinite": the first update overflows C, the shift cannot repair it, and the search stops after one
    generation with MaxIter's code and the state so far -- and the context goes on working."""
    c = A.repair_case(kind)
    ref = A.run_case(c, 6)
    assert ref["generations"] == gens and ref["chol_fixed"] == 1
    dev = device_run(va, c, MaxIter=6, trace=6)
    compare_trajectory(c, ref, dev, kind, gens)
    if kind == "indefinite":
        assert not np.all(np.isfinite(dev["C"])) and np.all(np.isfinite(dev["xmean"])) and dev["behind"] >= 1
        again = device_run(va, A.build_case("D2"), MaxIter=3, trace=3)
        assert again["generations"] == 3 and np.isfinite(again["fbest"])

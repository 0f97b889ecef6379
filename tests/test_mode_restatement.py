"""CPU: the NumPy restatement of the mode search (tests/_mode_ref.py), which tests/test_gpu_mode.py holds the device to, against
  * the 50-digit fixtures tests/golden/mp_mode_case*.json (tools/gen_mode_golden.py: the objective formed from the definitions, its
    gradient by numerical differentiation at 50 digits, the maximiser from every component mean by findroot): value and gradient to
    1e-12 relative, maximisers within 2 tol_grad |H^-1|_2 (both points have |grad g| <= tol_grad; H the restatement's own Hessian)
  * central differences of its own value (gradient) and gradient (Hessian)
  * closed forms: K = 1; two equal components closer than their width
  * SciPy's BFGS from the same starts, within the same bound
and the conditions the device cases rest on: from every start of every case of _mode_ref.CASES and of the edge posteriors the
restatement stops on the gradient, and the ranked values are at least 1e-6 apart (the duplicated component, bit-equal, aside)."""
import glob
import json
import os

import numpy as np
import pytest

from tests import _mode_ref as M

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp_mode_case*.json")))


def load(path):
    rec = json.load(open(path))
    vp = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, list) else v) for k, v in rec["vp"].items() if k != "trinfo"}
    tr = rec["vp"]["trinfo"]
    if tr is not None:
        tr = dict(tr)
        tr["lb_orig"] = np.array([-np.inf if v is None else v for v in tr["lb_orig"]])
        tr["ub_orig"] = np.array([np.inf if v is None else v for v in tr["ub_orig"]])
        for k in ("type", "mu", "delta", "scale", "R_mat"):
            tr[k] = None if tr[k] is None else np.asarray(tr[k])
    vp["trinfo"] = tr
    vp["D"], vp["K"] = int(vp["D"]), int(vp["K"])
    return vp, rec


def test_the_fixtures_cover_each_transform():
    assert len(GOLDEN) == 5
    seen, rot = set(), 0
    for path in GOLDEN:
        vp, rec = load(path)
        assert vp["D"] <= 3 and vp["K"] <= 4
        tr = vp["trinfo"]
        seen |= {None} if tr is None else set(int(t) for t in tr["type"])
        rot += tr is not None and tr["R_mat"] is not None and tr["scale"] is not None
    assert seen == {None, 0, 1, 2, 3} and rot >= 2


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_restatement_meets_the_fixtures(path):
    vp, rec = load(path)
    mu = np.asarray(vp["mu"]).reshape(vp["D"], vp["K"])
    for origflag in (0, 1):
        f = rec["flags"][str(origflag)]
        for p, val, grad in zip(rec["points"], f["value"], f["gradient"]):
            v, g = M.objective(vp, np.array(p), origflag, 1)
            val, grad = float(val), np.array([float(x) for x in grad])
            assert abs(v - val) <= 1e-12 * max(1.0, abs(val)), (path, origflag, v, val)
            assert np.max(np.abs(g - grad)) <= 1e-12 * max(1.0, np.max(np.abs(grad))), (path, origflag, g, grad)
        for k, (root, stop) in enumerate(zip(f["maximiser"], f["stop"])):
            r = M.bfgs(vp, mu[:, k], k, origflag)
            root = np.array([float(x) for x in root])
            H = M.objective(vp, root, origflag, 2)[2]
            assert r["stop"] == M.STOP_GRAD == stop and r["f"] >= r["f0"]
            assert np.max(np.abs(M.objective(vp, root, origflag, 1)[1])) <= 1e-12
            assert np.linalg.norm(r["u"] - root) <= M.distance_bound(H), (path, origflag, k, r["u"], root)
            ustar, _ = M.polish(vp, r["u"], origflag)
            assert np.linalg.norm(ustar - root) <= 1e-12 * max(1.0, np.linalg.norm(root))         # the polish lands on the 50-digit root


@pytest.mark.parametrize("name", ["d5k63_t1", "d13k64_t2", "d17k65_t3", "d4k65_all"])
def test_gradient_and_hessian_meet_central_differences(name):
    vp, _ = M.make_case(name)
    D = vp["D"]
    rng = np.random.default_rng(5)
    h = 1e-5
    for origflag in (0, 1):
        u = np.asarray(vp["mu"])[:, 1] + 0.1 * rng.normal(size=D)
        v, g, H = M.objective(vp, u, origflag, 2)
        gn = np.array([(M.objective(vp, u + h * e, origflag) - M.objective(vp, u - h * e, origflag)) / (2 * h) for e in np.eye(D)])
        Hn = np.array([(M.objective(vp, u + h * e, origflag, 1)[1] - M.objective(vp, u - h * e, origflag, 1)[1]) / (2 * h) for e in np.eye(D)])
        # central differences: truncation h^2 |f'''| / 6 and rounding eps |f| / h, both far below 1e-7 of the scale at h = 1e-5
        assert np.max(np.abs(g - gn)) <= 1e-7 * max(1.0, np.max(np.abs(g))), (name, origflag)
        assert np.max(np.abs(H - Hn)) <= 1e-7 * np.max(np.abs(H)), (name, origflag)
        assert np.array_equal(H, H.T) or np.max(np.abs(H - H.T)) <= 1e-12 * np.max(np.abs(H))


def test_closed_forms():
    # K = 1, origflag = 0: the mean, without an iteration
    vp = M.V.make_vp(4, 1, [0, 1, 2, 3], True, 11)
    r = M.mode(vp, 20, False)
    assert np.array_equal(r["us"][0], np.asarray(vp["mu"])[:, 0]) and r["iters"][0] == 0 and r["stop"][0] == M.STOP_GRAD
    assert np.array_equal(r["x"], r["us"][0]) and r["idx"] == 0
    # K = 1, origflag = 1, no rotation: type 0 keeps the mean (mapped), types 1 / 2 have v* = m - (sigma lambda)^2
    vp = M.V.make_vp(4, 1, [0, 1, 2, 0], False, 11)
    r = M.mode(vp, 20, True)
    m, sl2 = np.asarray(vp["mu"])[:, 0], (vp["sigma"][0] * np.ravel(vp["lambda"])) ** 2
    want = np.where(np.asarray(vp["trinfo"]["type"]) == 0, m, m - sl2)
    assert r["stop"][0] == M.STOP_GRAD and np.max(np.abs(r["us"][0] - want)) <= 2 * M.TOL_GRAD * np.max(sl2)
    assert np.allclose(r["x"], M.V.warp(want[None, :], "i", vp["trinfo"])[0], rtol=0, atol=1e-5)
    # two equal components at +-a e_1 with a < sigma lambda_1: the single mode at the midpoint, from both starts
    vp = M.make_merged_pair()
    r = M.mode(vp, 20, False)
    H = M.objective(vp, np.zeros(3), False, 2)[2]
    assert np.all(np.linalg.eigvalsh(H) < 0) and np.all(r["stop"] == M.STOP_GRAD)
    assert np.all(np.linalg.norm(r["us"], axis=1) <= M.distance_bound(H))


def _posteriors():
    for name in M.CASES:
        vp, nmax = M.make_case(name)
        yield name, vp, nmax
    yield "zero weight", M.make_zero_weight(), 20
    yield "isolated", M.make_isolated(), 20
    yield "duplicate", M.make_duplicate(), 5


def test_every_device_case_is_one_the_restatement_finishes():
    seen_D, seen_K, seen_n = set(), set(), set()
    for name, vp, nmax in _posteriors():
        D, K = vp["D"], vp["K"]
        seen_D.add(D), seen_K.add(K), seen_n.add(nmax if nmax < K else "all")
        for origflag in (0, 1):
            comps, f = M.rank_starts(vp, nmax, origflag)
            fs = np.sort(f)
            gaps = np.diff(fs)
            if name == "duplicate":
                assert f[2] == f[5] and {2, 5} <= set(comps.tolist())
                gaps = np.diff(np.unique(fs))
            assert gaps.size == 0 or gaps.min() >= 1e-6, (name, origflag, gaps.min())
            r = M.mode(vp, nmax, origflag)
            assert np.all(r["stop"] == M.STOP_GRAD), (name, origflag, r["stop"])
            assert np.all(r["fs"] >= r["f0"]) and np.all(np.isfinite(r["fs"]))
    assert {1, 4, 5, 13, 17, 25, 32} <= seen_D and {1, 2, 63, 64, 65, 130, 512} <= seen_K and {1, 5, 20, "all"} <= seen_n
    vp = M.make_isolated()                        # 40 sigma lambda away: the other components' densities underflow there
    u = np.asarray(vp["mu"])[:, 4]
    assert M.logq(dict(vp, K=4, mu=np.asarray(vp["mu"])[:, :4], sigma=vp["sigma"][:4], w=vp["w"][:4]), u) < -744.5
    assert M.make_zero_weight()["w"][1] == 0.0


@pytest.mark.parametrize("name", ["d4k65_all", "d5k63_t1", "d17k65_t3"])
def test_scipy_bfgs_lands_on_the_same_maxima(name):
    from scipy.optimize import minimize

    vp, nmax = M.make_case(name)
    mu = np.asarray(vp["mu"])
    for origflag in (0, 1):
        r = M.mode(vp, nmax, origflag)
        compared = 0
        for s, c in enumerate(r["start_comp"][:8]):
            fun = lambda u: tuple(-x for x in M.objective(vp, u, origflag, 1))      # noqa: E731
            sp = minimize(fun, mu[:, c], jac=True, method="BFGS", options={"gtol": M.TOL_GRAD})
            ua, Ha = M.polish(vp, r["us"][s], origflag)
            ub, _ = M.polish(vp, sp.x, origflag)
            if np.linalg.norm(ua - ub) > 1e-9:       # another local maximum (a different line search may cross a saddle): nothing to compare
                continue
            compared += 1
            assert np.linalg.norm(r["us"][s] - sp.x) <= M.distance_bound(Ha) * max(1.0, np.max(np.abs(sp.jac)) / M.TOL_GRAD), (name, origflag, s)
        assert 4 * compared >= 3 * min(8, len(r["start_comp"])), (name, origflag, compared)

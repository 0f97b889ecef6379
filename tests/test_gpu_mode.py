"""GPU: vbmc_vp_mode through vbmc_amd.vptools.vbmc_mode(..., details=True) against the NumPy restatement tests/_mode_ref.py, by
properties and not by trajectory: near convergence the line search decides on differences at rounding level, so the device and the
restatement may legitimately take different steps to the same maximum.

For every start of every case (tests/test_mode_restatement.py checks on the CPU that the restatement itself stops on the gradient from
every start of every case, and that the ranked values are at least 1e-6 apart):
  a. fs (f0) is the restatement's objective at the returned us (at the start) within PDF_TOL max(1, |ref|), the bound
     tests/test_gpu_vptools.py holds vbmc_vp_pdf's log density to
  b. stop is GRAD and the restatement's max |grad g(us)| <= tol_grad + the gradient's own rounding (32 eps times the sum of the
     magnitudes of the terms the gradient is made of)
  c. fs >= f0
  d. |us - u*|_2 <= 2 tol_grad |H^-1|_2 with u* the restatement's Newton-polished maximiser from us and H its Hessian there
  e. xs is us (origflag = 0), or what vbmc_vp_rnd's kernel makes of us, to the bit: a draw with zero normals from a mixture whose
     means are the rows of us
  f. start_comp is the restatement's stable order
  g. idx, x and fval follow the winner rule from the returned fs
Cases: D = 1, 4, 5, 13, 17, 25, 32 (each padded width and its padding), K = 1, 2, 63, 64, 65, 130, 512 (the lane seams, several
components per lane, the maximum), nmax = 1, 5, 20 and >= K, both flags, no transform, each type alone, all four with scale and
rotation; a zero-weight component among the starts, a component 40 sigma lambda from the others, two identical components, the merged
pair, K = 1 to the bit."""
import numpy as np
import pytest

from tests import _mode_ref as M

pytestmark = pytest.mark.gpu
PDF_TOL = 2.7e-13          # tests/test_gpu_vptools.py: PDF_TOL["gauss"]
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def V():
    from vbmc_amd import vptools

    return vptools


def grad_rounding(vp, u, origflag):
    """32 eps times the largest sum of magnitudes a gradient entry is made of"""
    D, K, mu, sigma, lam, w = M._parts(vp)
    prec = 1.0 / (sigma[:, None] * lam[None, :]) ** 2
    with np.errstate(divide="ignore"):
        a = np.log(w) - D * np.log(sigma) - 0.5 * np.sum((u - mu) ** 2 * prec, axis=1)
    r = np.exp(a - a.max())
    r /= r.sum()
    scale = np.max(r @ ((np.abs(u) + np.abs(mu)) * prec))
    t = M._transform(vp)
    if origflag and t is not None:
        scale += np.max(np.abs(t[3]).T @ np.maximum(1.0, np.abs(t[2])))
    return 32 * EPS * scale


def rows_through_rnd(V, vp, us):
    """The rows of us through vbmc_vp_rnd's inverse transform and clamp: row i is drawn from component i of a mixture whose means
    are the rows of us, with zero normals"""
    S, D = us.shape
    q = dict(vp, K=S, mu=us.T.copy(), sigma=np.ones(S), w=np.full(S, 1.0 / S))
    B = np.zeros((S, D + 1))
    B[:, 0] = (np.arange(S) + 0.5) / S
    X, I = V.vbmc_rnd(q, S, True, False, block=B)
    assert np.array_equal(I, np.arange(S))
    return X


def check(V, vp, nmax, origflag, tag, tol_grad=M.TOL_GRAD):
    x, det = V.vbmc_mode(vp, nmax, origflag, details=True, tol_grad=tol_grad)
    D, K, mu, *_ = M._parts(vp)
    comps, f_all = M.rank_starts(vp, nmax, origflag)
    S = len(comps)
    assert det["S"] == S and det["us"].shape == (S, D), tag
    assert np.array_equal(det["start_comp"], comps), (tag, det["start_comp"], comps)                                   # f
    worst = dict(a=0.0, b=0.0, d=0.0)
    for s in range(S):
        us = det["us"][s]
        ref, ref0 = M.objective(vp, us, origflag), f_all[comps[s]]
        ea, e0 = abs(det["fs"][s] - ref) / max(1.0, abs(ref)), abs(det["f0"][s] - ref0) / max(1.0, abs(ref0))
        worst["a"] = max(worst["a"], ea, e0)
        assert ea <= PDF_TOL and e0 <= PDF_TOL, (tag, s, ea, e0)                                                         # a
        g = M.objective(vp, us, origflag, 1)[1]
        worst["b"] = max(worst["b"], float(np.max(np.abs(g))))
        assert det["stop"][s] == M.STOP_GRAD, (tag, s, det["stop"][s], det["iters"][s])                                  # b
        assert np.max(np.abs(g)) <= tol_grad + grad_rounding(vp, us, origflag), (tag, s, np.max(np.abs(g)))
        assert det["fs"][s] >= det["f0"][s], (tag, s)                                                                    # c
        ustar, H = M.polish(vp, us, origflag)
        dist, bound = float(np.linalg.norm(us - ustar)), M.distance_bound(H, tol_grad)
        worst["d"] = max(worst["d"], dist / bound)
        assert dist <= bound, (tag, s, dist, bound)                                                                      # d
        assert 0 <= det["iters"][s] <= M.MAX_ITER and det["nfev"][s] >= 1 + det["iters"][s], (tag, s)
    if origflag and vp.get("trinfo"):
        assert np.array_equal(det["xs"], rows_through_rnd(V, vp, det["us"])), tag                                        # e
        lo, hi = M.V.clamp_ends(vp["trinfo"])
        assert np.all(det["xs"] >= lo) and np.all(det["xs"] <= hi), tag
    else:
        assert np.array_equal(det["xs"], det["us"]), tag
    idx = M.winner(det["fs"])
    assert det["idx"] == idx and det["fval"] == det["fs"][idx] and np.array_equal(x, det["xs"][idx]), tag               # g
    print("MODE-MEASURE %s a %.2e b %.2e d/bound %.2e iters max %d" % (tag, worst["a"], worst["b"], worst["d"], det["iters"].max()))
    return x, det


@pytest.mark.parametrize("origflag", [0, 1])
@pytest.mark.parametrize("name", list(M.CASES))
def test_properties_of_every_start(V, name, origflag):
    vp, nmax = M.make_case(name)
    check(V, vp, nmax, origflag, "%s of=%d" % (name, origflag))


@pytest.mark.parametrize("origflag", [0, 1])
def test_edge_posteriors(V, origflag):
    x, det = check(V, M.make_zero_weight(), 20, origflag, "zero weight of=%d" % origflag)
    assert 1 in det["start_comp"]
    vp = M.make_isolated()
    x, det = check(V, vp, 20, origflag, "isolated of=%d" % origflag)
    assert np.all(np.isfinite(det["f0"])) and np.all(np.isfinite(det["fs"]))
    if not origflag:                                          # alone in its neighbourhood: the start is the maximum
        assert det["iters"][4] == 0 and np.array_equal(det["us"][4], np.asarray(vp["mu"])[:, 4])
    vp = M.make_duplicate()
    x, det = check(V, vp, 5, origflag, "duplicate of=%d" % origflag)
    at = [int(np.flatnonzero(det["start_comp"] == c)[0]) for c in (2, 5)]
    assert at[1] == at[0] + 1 and det["f0"][at[0]] == det["f0"][at[1]]                 # bit-equal values come out in index order
    assert np.array_equal(det["us"][at[0]], det["us"][at[1]]) and det["fs"][at[0]] == det["fs"][at[1]]


def test_closed_forms(V):
    # K = 1, origflag = 0: the mean itself, to the bit, without an iteration
    vp, _ = M.make_case("d4k2_t0")
    one = dict(vp, K=1, mu=np.asarray(vp["mu"])[:, :1].copy(), sigma=np.asarray(vp["sigma"])[:1], w=np.ones(1))
    x, det = V.vbmc_mode(one, 20, False, details=True)
    assert np.array_equal(x, one["mu"][:, 0]) and det["iters"][0] == 0 and det["stop"][0] == M.STOP_GRAD and det["S"] == 1
    # K = 1, origflag = 1, no rotation: type 0 maps the mean, types 1 / 2 have v* = m - (sigma lambda)^2
    vp = M.V.make_vp(4, 1, [0, 1, 2, 0], False, 11)
    x, det = check(V, vp, 20, True, "K=1 closed form")
    m, sl2 = np.asarray(vp["mu"])[:, 0], (vp["sigma"][0] * np.ravel(vp["lambda"])) ** 2
    want = np.where(np.asarray(vp["trinfo"]["type"]) == 0, m, m - sl2)
    assert np.max(np.abs(det["us"][0] - want)) <= 2 * M.TOL_GRAD * np.max(sl2), (det["us"][0], want)
    assert np.allclose(x, M.back(vp, want, True)[0], rtol=1e-5)
    # two equal components at +-a e_1 with a < sigma lambda_1: one mode at the midpoint, from both starts
    vp = M.make_merged_pair()
    x, det = check(V, vp, 20, False, "merged pair")
    H = M.objective(vp, np.zeros(3), False, 2)[2]
    assert np.all(np.linalg.norm(det["us"], axis=1) <= M.distance_bound(H))


def test_repeat_null_outputs_and_refusals(V):
    from vbmc_amd import VbmcHipError, VbmcUnsupported

    vp, nmax = M.make_case("d25k130_mix")
    x1, d1 = V.vbmc_mode(vp, nmax, True, details=True)
    x2, d2 = V.vbmc_mode(vp, nmax, True, details=True)
    assert np.array_equal(x1, x2) and all(np.array_equal(d1[k], d2[k]) for k in d1)          # a repeated call is bit-identical
    assert np.array_equal(V.vbmc_mode(vp, nmax, True), x1)                                     # every optional pointer NULL
    x3, vp3 = V.vbmc_mode(vp, nmax, True, nargout=2)
    assert np.array_equal(vp3["mode"], x1) and "mode" not in vp
    assert np.array_equal(V.vbmc_mode(vp3), x1)                                                # the stored mode (no device call)
    assert "mode" not in V.vbmc_mode(vp, nmax, False, nargout=2)[1]                            # stored for origflag only
    bad = dict(vp, trinfo=dict(vp["trinfo"], type=np.where(np.arange(25) == 3, 7, vp["trinfo"]["type"])))
    with pytest.raises(VbmcUnsupported):
        V.vbmc_mode(bad, nmax, True)
    nan = dict(vp, mu=np.where(np.arange(25 * 130).reshape(25, 130) == 77, np.nan, vp["mu"]))
    for kw, v in ((dict(), nan), (dict(tol_grad=0.0), vp), (dict(tol_grad=float("nan")), vp), (dict(max_iter=1001), vp)):
        with pytest.raises(VbmcHipError) as e:
            V.vbmc_mode(v, nmax, True, **kw)
        assert e.value.status == 1 and not isinstance(e.value, VbmcUnsupported), kw
        assert np.array_equal(V.vbmc_mode(vp, nmax, True), x1)                                 # a working call on the same context
    # max_iter is honoured and reported
    vpl, nl = M.make_case("d4k65_all")
    _, det = V.vbmc_mode(vpl, nl, True, details=True, max_iter=2)
    assert set(det["stop"].tolist()) <= {M.STOP_GRAD, M.STOP_MAXITER} and M.STOP_MAXITER in det["stop"] and det["iters"].max() == 2
    assert np.all(det["fs"] >= det["f0"])

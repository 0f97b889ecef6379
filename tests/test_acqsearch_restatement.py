"""CPU: properties of the NumPy restatement tests/_acqsearch_ref.py of the device-resident acquisition search -- what the GPU test
tests/test_gpu_acqsearch.py holds the device against -- and the rank-gap precondition of that comparison."""
import numpy as np
import pytest

from tests import _acqsearch_ref as A


def quad(X):
    return np.sum((np.asarray(X) - np.array([0.3, -0.2, 0.1])[None, :]) ** 2 * np.array([1.0, 10.0, 100.0])[None, :], axis=1)


def run(fun, D=3, seed=0, G=2000, **kw):
    rng = np.random.default_rng(seed)
    lam = kw.get("popsize") or A.default_popsize(D)
    args = dict(TolX=1e-12, TolFun=1e-14, TolHistFun=1e-15, Z=rng.standard_normal((D, lam, G)))
    args.update(kw)
    x0 = args.pop("x0", np.full(D, 0.5))
    insigma = args.pop("insigma", np.full(D, 0.3))
    return A.cmaes_chol(fun, x0, insigma, np.full(D, -1.0), np.full(D, 1.0), **args)


def test_factor_reproduces_the_covariance_and_points_stay_in_the_box():
    r = run(quad, MaxIter=60)
    Cprev = np.diag(np.ones(3))
    for t in r["trace"]:
        assert np.max(np.abs(t["A"] @ t["A"].T - Cprev)) <= 1e-14 * np.max(np.abs(Cprev))
        assert np.array_equal(t["A"], np.tril(t["A"])) and np.all(np.diag(t["A"]) > 0)
        assert np.all(t["X"] >= -1.0) and np.all(t["X"] <= 1.0)
        assert np.array_equal(t["C"], t["C"].T)
        Cprev = t["C"]
    assert r["generations"] == 60 and r["stop"] == "MaxIter" and r["evals"] == 60 * r["popsize"]


def test_separable_quadratic_is_minimised():
    r = run(quad)
    assert r["fbest"] < 1e-6 and np.max(np.abs(r["xbest"] - np.array([0.3, -0.2, 0.1]))) < 1e-3
    assert r["stop"] in ("TolX", "TolFun", "TolHistFun")


def test_every_stop_code_is_reachable():
    assert run(quad, insigma=np.full(3, 1e-9), TolX=1e-6)["stop"] == "TolX"
    flat = run(lambda X: np.zeros(np.asarray(X).shape[0]), TolX=0.0, TolFun=1e-12, TolHistFun=0.0)
    assert flat["stop"] == "TolFun" and flat["generations"] == 3
    hist = run(lambda X: np.zeros(np.asarray(X).shape[0]), TolX=0.0, TolFun=0.0, TolHistFun=1e-13)
    assert hist["stop"] == "TolHistFun" and hist["generations"] == A.constants(3, 7)["nh"] + 1
    few = run(quad, MaxFunEvals=30)
    assert few["stop"] == "MaxFunEvals" and few["evals"] == few["generations"] * few["popsize"] == 35
    assert run(quad, MaxIter=4)["stop"] == "MaxIter"
    with pytest.raises(ValueError, match="normal block exhausted"):
        run(quad, G=5, MaxIter=9)


def test_values_that_are_not_finite_rank_last_and_ties_keep_the_index_order():
    def fun(X):
        f = np.zeros(np.asarray(X).shape[0])
        f[0] = np.nan
        f[2] = -np.inf
        return f

    t = run(fun, MaxIter=1)["trace"][0]
    assert list(t["order"]) == [1, 3, 4, 5, 6, 0, 2] and np.all(np.isinf(t["F"][-2:]))


def test_start_on_a_face_is_clamped():
    r = run(quad, x0=np.array([1.0, -1.0, 0.0]), MaxIter=5)
    X = r["trace"][0]["X"]
    assert np.any(X[0] == 1.0) and np.any(X[1] == -1.0) and np.all(np.abs(X) <= 1.0)


@pytest.mark.parametrize("name", sorted(A.search_cases()))
def test_rank_gap_precondition_of_the_gpu_trajectory_test(name):
    """Every generation the GPU test compares: neighbouring sorted values further apart than 1e-6 (1 + |F|), all values finite."""
    c = A.build_case(name)
    r = A.run_case(c, 20)
    assert r["generations"] == 20 and len(r["trace"]) == 20
    assert all(np.all(np.isfinite(t["F"])) for t in r["trace"])
    assert A.min_rank_gap(r["trace"]) > 1e-6
    D, N, S, K, acq, reg, face, _ = A.search_cases()[name]
    assert c["gp"]["X"].shape == (N, D) and len(c["gp"]["post"]) == S and c["vp"]["K"] == K and c["lam"] == A.default_popsize(D)
    if face:
        assert c["x0"][0] == c["UB"][0] and c["x0"][-1] == c["LB"][-1]


def test_the_cases_cover_the_edges():
    cs = A.search_cases().values()
    assert {c[0] for c in cs} >= {2, 3, 10, 32} and {c[1] for c in cs} == {17, 40, 1264} and {c[2] for c in cs} == {1, 3}
    assert {c[3] for c in cs} == {1, 2} and {c[4] for c in cs} == {"acqf", "acqflog", "acqus", "acqfsn2"}
    assert {c[5] for c in cs} == {True, False} and any(c[6] for c in cs)
    assert A.default_popsize(2) == 6 and A.default_popsize(32) == 14


def test_covariance_repair_shift_and_stop():
    """A singular C is shifted by 1e-14 max diag once and the search goes on; a C that the shift cannot repair stops the search with
    MaxIter's code and the state so far.  Both on a plain quadratic, then on the two cases the GPU test compares (with their rank gap)."""
    r = run(quad, insigma=np.array([0.3, 1e-170, 0.3]), MaxIter=5)
    assert r["chol_fixed"] == 1 and r["generations"] == 5 and np.all(np.isfinite(r["C"]))
    A0 = r["trace"][0]["A"]
    assert abs(A0[1, 1] - 1e-7) < 1e-20 and A0[0, 0] == np.sqrt(1.0 + 1e-14)      # the shift goes onto the whole diagonal
    rng = np.random.default_rng(0)
    bad = A.cmaes_chol(quad, np.full(3, 0.5), np.full(3, 1e-300), np.full(3, -1.0), np.full(3, 1.0), TolX=0.0, TolFun=0.0, TolHistFun=0.0,
                       MaxIter=9, Z=1e300 * rng.standard_normal((3, 7, 9)))
    assert bad["generations"] == 1 and bad["stop"] == "MaxIter" and bad["chol_fixed"] == 1 and not np.all(np.isfinite(bad["C"]))
    assert np.all(np.isfinite(bad["xmean"])) and np.all(np.abs(bad["xmean"]) <= 1.0) and bad["evals"] == 7
    for kind, gens in (("shift", 6), ("indefinite", 1)):
        rr = A.run_case(A.repair_case(kind), 6)
        assert rr["generations"] == gens and rr["stop"] == "MaxIter" and rr["chol_fixed"] == 1
        assert A.min_rank_gap(rr["trace"]) > 1e-6

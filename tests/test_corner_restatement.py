"""CPU: the restatement tests/_corner_ref.py of cornerplot.m:113-156 / kde2d.m / quantile1.m, and the conditions tests/test_gpu_corner.py
relies on for each of its cases, checked on the restatement's own draws (tests/_vptools_ref.rnd on the dumped block):
  * root() arrives at a bracket, and a 2000-point scan of t - evolve(t) over it shows exactly one sign change, so that "the root" is
    one number (a case that failed either would be replaced, not tolerated);
  * the small cut case has no bracket below 0.1 (the refusal).
The analytic anchor: the kde2d density of Ns = 1e5 draws of a 2-D standard normal on res = 64 against the normal density at the mesh
points, over the seeds below: the worst max |ref - true| / peak was ANALYTIC_WORST (Monte-Carlo and bandwidth error); three times it
is held here and by the device test."""
import numpy as np
import pytest

from tests import _corner_ref as R

ANALYTIC_WORST = 5.621e-2      # measured: 4.319e-2, 5.621e-2, 4.240e-2 (the 64-point grid spans the samples' whole range, +-4.5)
ANALYTIC_SEEDS = (11, 12, 13)


def analytic_error(X, density, bounds):
    """max |density - true| / peak for samples of a 2-D standard normal"""
    x, y = (np.linspace(bounds[d, 0], bounds[d, 1], density.shape[0]) for d in (0, 1))          # kde2d.m:105
    true = np.exp(-0.5 * (x[None, :] ** 2 + y[:, None] ** 2)) / (2 * np.pi)                      # row the d2 mesh, column the d1 mesh
    return float(np.max(np.abs(density - true)) / np.max(true))


def test_restatement_against_the_normal_density():
    worst = 0.0
    for seed in ANALYTIC_SEEDS:
        X = np.random.default_rng(seed).normal(size=(100000, 2))
        out = R.corner(X, None, 64, 40, ())
        e = analytic_error(X, out["density"][0], out["bounds"])
        print("CORNER-MEASURE analytic seed=%d err=%.4e bandwidth=%s" % (seed, e, out["bandwidth"][0]))
        worst = max(worst, e)
    print("CORNER-MEASURE analytic worst %.4e" % worst)
    assert worst <= 3 * ANALYTIC_WORST, worst


@pytest.mark.parametrize("n", (16, 32, 64))
def test_transform_convention(n):
    r = np.random.default_rng(3)
    x = r.random((n, n))
    x /= x.sum()
    a = R.dct2d(x)
    assert np.max(np.abs(a - R.dct2d_sum(x))) <= 1e-13 * np.max(np.abs(a))
    b = R.idct2d_sum(a)
    assert np.max(np.abs(R.idct2d(a) - b)) <= 1e-13 * np.max(np.abs(b))
    assert np.max(np.abs(R.idct2d(a) - x.T)) <= 1e-14                                 # the pair inverts, up to idct2d's one transpose
    u = r.random((n, n))                                                              # unequal directions: which index is which
    assert np.max(np.abs(R.idct2d(u) - R.idct2d_sum(u))) <= 1e-13 * n


def test_the_memoised_dag_is_the_recursion():
    X, res, b = R.case_draws("three32")
    k = R.corner(X, b, res, 40, ())["kde"][1]
    for t in (0.0, 1e-4, k["tstar"], 0.03):
        dag = R.func_dag(t, k["N"], k["I"], k["A2"])
        assert len(dag) == 18
        for s in ((0, 2), (2, 0), (1, 1), (3, 1), (0, 5)):
            count = [0]
            assert R.func(s, t, k["N"], k["I"], k["A2"], count) == dag[s], (s, t)
            assert count[0] == 2 ** (6 - sum(s)) - 1                                  # the recursion visits a node many times
        plain = R.evolve(t, k["N"], k["I"], k["A2"], f=R.func)
        assert plain == R.evolve(t, k["N"], k["I"], k["A2"]), t


def test_ndhist_against_histogram2d():
    X, b = R.edge_matrix()
    M = 16
    t = (X - b[None, :, 0]) / (b[:, 1] - b[:, 0])[None, :]
    binned, counts = R.ndhist(t, M)
    inside = np.all((X >= b[None, :, 0]) & (X <= b[None, :, 1]), axis=1)
    assert 0 < inside.sum() < X.shape[0] - 2
    ref, _, _ = np.histogram2d(t[inside, 0], t[inside, 1], bins=[np.arange(M + 1) / M] * 2)      # the last bin is closed, as min(bins, M) makes it
    assert np.array_equal(counts, ref.astype(np.int64))
    assert counts.sum() == inside.sum()
    assert counts[M - 1, :].sum() >= 2 and counts[:, M - 1].sum() >= 2 and counts[0, :].sum() >= 2   # rows on the bounds are counted
    assert np.array_equal(binned, counts * (1 / X.shape[0]))                          # the dropped rows still count in N
    assert abs(binned.sum() - inside.sum() / X.shape[0]) < 1e-15
    tt = np.array([0.0, 1.0, -1e-300, 1 + 1e-15, np.nan, 0.5, 1 / M, np.nextafter(1 / M, 0)])
    assert R.ndhist_bins(tt, M).tolist() == [1, M, 0, 0, 0, M // 2 + 1, 2, 1]


def test_hist1_edges():
    x = np.array([0.0, 1.0, 0.25, 0.2499999, 0.999, -0.1, 1.1, 0.5])
    assert R.hist1(x, 0.0, 1.0, 4).tolist() == [2, 1, 1, 2]


def _sorted_quantile(x, p):
    """quantile1's rule written on the sorted column with explicit ranks"""
    x = np.sort(x)
    n = x.size
    out = []
    for q in np.atleast_1d(p):
        r = q * n
        k = int(np.floor(r + 0.5))
        r -= k
        lo, hi = x[max(k, 1) - 1], x[min(k + 1, n) - 1]
        out.append(lo if (r == -0.5 or lo == hi) else (0.5 + r) * hi + (0.5 - r) * lo)
    return np.array(out)


@pytest.mark.parametrize("n", (10, 11, 1003))
def test_quantiles(n):
    r = np.random.default_rng(n)
    x = r.normal(size=n)
    s = np.sort(x)
    med = R.quantile1(x, 0.5)[0]
    assert med == (s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2) == np.median(x)
    p = np.array(R.QUANT_P + (0.5 / n / 2, 0.3))
    got = R.quantile1(x, p)
    assert np.array_equal(got, _sorted_quantile(x, p))
    assert got[4] == s[0] and got[5] == s[-1] and got[7] == s[0]                      # p = 0, p = 1, p below 0.5 / n
    assert got[0] == med                                                              # 0.5 through the general branch
    ties = np.round(x * 2) / 2                                                        # many repeated values
    got = R.quantile1(ties, p)
    assert np.array_equal(got, _sorted_quantile(ties, p)) and np.all(np.isin(got, ties) | (p == 0.3))
    k, kp1, rr = R.quantile_ranks(p, n)
    assert np.all(k >= 1) and np.all(kp1 <= n) and np.all(kp1 - k <= 1)


_cond = {}


@pytest.mark.parametrize("name", R.VP_CASES + ("edge",))
def test_conditions_of_the_gpu_cases(name):
    X, res, b = (R.edge_matrix()[0], 32, R.edge_matrix()[1]) if name == "edge" else R.case_draws(name)
    out = R.corner(X, b, res, 40, R.QUANT_P)                                          # NoBracket would fail the case
    if name != "one":
        assert len(out["pairs"]) == X.shape[1] * (X.shape[1] - 1) // 2 > 0
    pairs = range(len(out["pairs"])) if name != "wide32" else range(0, 496, 31)      # (a sixteenth of the 496 pairs are scanned)
    for pp in pairs:
        k = out["kde"][pp]
        ts = np.linspace(0.0, out["tol"][pp], 2000)
        f = np.array([k["f"](t) for t in ts])
        assert np.all(np.isfinite(f)), (name, pp)
        assert int(np.sum(np.sign(f[1:]) != np.sign(f[:-1]))) == 1, (name, pp)
    if name in ("cut0", "cut1", "edge"):
        inside = np.all((X >= out["bounds"][None, :, 0]) & (X <= out["bounds"][None, :, 1]), axis=1)
        assert out["counts2"].sum(axis=(1, 2)).max() < X.shape[0] and inside.sum() < X.shape[0]
    if name == "pile":
        lo = np.min(X[:, 0])
        assert np.sum(X[:, 0] == lo) > 50 and np.sum(X[:, 0] == np.max(X[:, 0])) > 50     # ties for the selection


def test_the_small_cut_case_has_no_bracket():
    X, b = R.small_cut()
    with pytest.raises(R.NoBracket):
        R.corner(X, b, 64, 40, ())
    assert 0.05 < np.mean(np.all((X >= b[None, :, 0]) & (X <= b[None, :, 1]), axis=1)) < 0.5


def test_zero_range_column():
    X = np.random.default_rng(5).normal(size=(500, 3))
    X[:, 1] = 1.0
    out = R.corner(X, None, 16, 40, (0.5,))
    assert np.all(out["hist"][1] == 0) and out["hist"][0].sum() == 500
    assert np.all(np.isnan(out["tstar"][[0, 2]])) and np.isfinite(out["tstar"][1])    # pairs (0, 1) and (1, 2) hold the column
    assert out["quant"][1, 0] == 1.0

"""CPU: the restatement tests/_mtv_ref.py of vbmc_mtv.m / kde1d.m / qtrapz.m, and the conditions that tests/test_gpu_mtv.py relies on
for each of its cases (tests/_mtv_ref.make_pair), checked on the restatement's own draws (tests/_vptools_ref.rnd on the dumped block,
which the device equals to 8.9e-15):
  * in the final bracket of root() a 400-point scan of fixed_point shows exactly one sign change, so that "the root" is one number;
  * length(unique(data)) equals the device's clamp-end rule in every column;
  * no column has zero range (the degenerate case apart, which has exactly one).
The analytic check: two one-component posteriors with the identity transform and unit scale, means 0 and m, have the marginal total
variation erf(m / (2 sqrt 2)).  The restatement at Ns = 1e5 was measured against it over the five seeds below: the worst error was
ANALYTIC_WORST (Monte-Carlo and bandwidth error); three times it is held here and by the device test."""
import math

import numpy as np
import pytest

from tests import _mtv_ref as M
from tests import _vptools_ref as T

ANALYTIC_WORST = 7.227e-3      # measured: 7.227e-3 (m = 0), 3.451e-3 (m = 0.5), 4.121e-3 (m = 2)
ANALYTIC_SEEDS = (11, 12, 13, 14, 15)
ANALYTIC_MEANS = (0.0, 0.5, 2.0)


def analytic(m):
    return math.erf(m / (2 * math.sqrt(2)))


def draws(vp, Ns, seed, block_seed=None):
    """vbmc_rnd(vp, Ns, 1, 1) by the restatement on the block that ``seed`` (or ``block_seed``) stands for (a host function: no device)"""
    from vbmc_amd import vptools

    B, _ = vptools.vp_rnd_rng_dump(seed if block_seed is None else block_seed, Ns, vp["D"], vp["w"], True)
    return T.rnd(vp, Ns, True, True, B, seed)[0]


_cache = {}


def pair_draws(name):
    if name not in _cache:
        vp1, vp2, Ns, nkde, nquad, same = M.make_pair(name)
        xx1 = draws(vp1, Ns, M.SEED)
        xx2 = draws(vp2, Ns, M.SEED + 1, M.SEED if same else None)
        _cache[name] = (vp1, vp2, xx1, xx2, nkde, nquad)
    return _cache[name]


@pytest.mark.parametrize("m", ANALYTIC_MEANS)
def test_restatement_against_the_analytic_value(m):
    worst = 0.0
    for seed in ANALYTIC_SEEDS:
        xx1, xx2 = draws(M._gauss(1, 0.0, 1.0), 100000, seed), draws(M._gauss(1, m, 1.0), 100000, seed + 1)
        inf = np.array([np.inf])
        got, _ = M.mtv(xx1, xx2, -inf, inf, -inf, inf)
        worst = max(worst, abs(got[0] - analytic(m)))
        print("MTV-MEASURE analytic m=%g seed=%d mtv=%.6f exact=%.6f" % (m, seed, got[0], analytic(m)))
    print("MTV-MEASURE analytic m=%g worst %.3e" % (m, worst))
    assert worst <= 3 * ANALYTIC_WORST, (m, worst)


def test_transform_convention():
    r = np.random.default_rng(3)
    x = r.random(256)
    x /= x.sum()
    a = M.dct1d(x)
    assert np.max(np.abs(a - M.dct_sum(x))) <= 1e-13 * np.max(np.abs(a))
    assert np.max(np.abs(M.idct1d(a) - M.idct_sum(a))) <= 1e-13 * np.max(np.abs(M.idct_sum(a)))
    assert np.max(np.abs(M.idct1d(a) - 256 * x)) <= 1e-12                             # the pair inverts up to the factor n (kde1d.m:58 divides by R only)


@pytest.mark.parametrize("name", M.PAIRS)
def test_conditions_of_the_gpu_cases(name):
    vp1, vp2, xx1, xx2, nkde, nquad = pair_draws(name)
    D = vp1["D"]
    _, st = M.mtv(xx1, xx2, *M.bounds_of(vp1, D), *M.bounds_of(vp2, D), nkde=nkde, nquad=2)
    for p, (vp, xx) in enumerate(((vp1, xx1), (vp2, xx2))):
        lb, ub = M.bounds_of(vp, D)
        for d in range(D):
            col = xx[:, d]
            assert np.max(col) > np.min(col), (name, p, d)
            assert np.unique(col).size == M.clamp_rule(col, lb[d], ub[d]) == st["nuniq"][p, d], (name, p, d)
            k = st["kde"][p][d]
            ts = np.linspace(0.0, st["tol"][p, d], 400)
            f = np.array([M.fixed_point(t, k["N"], k["I"], k["a2"]) for t in ts])
            assert np.all(np.isfinite(f)), (name, p, d)
            assert int(np.sum(np.sign(f[1:]) != np.sign(f[:-1]))) == 1, (name, p, d)
    if name == "pile":
        assert st["nuniq"][0, 0] < xx1.shape[0] and st["tstar"][0, 0] < 1e-6, (st["nuniq"], st["tstar"])


def test_the_degenerate_column_has_zero_range():
    vp = M.make_degenerate()
    xx = draws(vp, 1003, M.SEED)
    rng = np.max(xx, axis=0) - np.min(xx, axis=0)
    assert rng[1] == 0 and rng[0] > 0 and rng[2] > 0
    got, _ = M.mtv(xx, draws(vp, 1003, M.SEED + 1), *M.bounds_of(vp, 3), *M.bounds_of(vp, 3), nkde=256, nquad=1000)
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))


@pytest.mark.parametrize("Ns, seed", ((5, M.SEED), (20, 101)))
def test_few_draws_reach_the_fminbnd_branch(Ns, seed):
    """(At Ns = 5 every seed tried ends there; at Ns = 20 it depends on the draws: of the seeds 100 .. 105, 101 and 105 do.)"""
    xx = draws(M._gauss(1, 0.0, 1.0), Ns, seed)
    lo, hi = M.mesh_bounds(xx, -np.inf, np.inf)
    with pytest.raises(M.NoBracket):
        M.kde1d(xx[:, 0], 256, lo[0], hi[0])

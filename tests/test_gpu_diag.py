"""GPU: vbmc_vp_diagnostics (vbmc_amd.vptools.vp_diagnostics / vbmc_diagnostics) against the restatements fed the device's own draws.

Runs are tests/_diag_ref.runs: make_case(X) and its siblings.  Ns = 1003, nkde = 256, nquad = 1000 unless the case says otherwise.
Identical: run i's draws against vbmc_vp_rnd(vp_i, Ns, 1, 1, seed + i); mesh, counts and nuniq against tests/_mtv_ref.mtv on the two
runs' sample matrices with infinite bounds and the clamp-end unique count (which the test finds equal to np.unique in every column);
the symmetry of mtv and maxmtv_mat; a repeated call; a run's stage outputs in a call of four runs and in a call of two.
kl_mat against tests/_vptools_ref.kldiv_terms on those draws within the project's 1e-10 max(1, |kl|).
Tolerances of tstar, density and mtv.  They were not fixed in advance: each is ten times the largest deviation measured over the cases
(DESIGN.md section 6k lists the measurements) and sits below the project's 1e-10 for values.
  tstar    |dev - ref| <= TSTAR_TOL |ref|
  density  |dev - ref| <= DENS_TOL max(ref)
  mtv      |dev - ref| <= MTV_TOL
The cosine transform is k_diag_dct, not vbmc_vp_mtv's k_mtv_dct (another order of summation), so two runs without a trinfo agree with
vbmc_vp_mtv in draws, mesh, counts and nuniq to the bit and in tstar, density and mtv within these tolerances.

Next to underflow (the runs of make_case("B", width=0.08): some hundred of the 6 x 1003 cross densities lie below realmin) the
reference's density is what rounding to a few bits left of it, and k_diag_cross_kl forms it as the reference does; vbmc_vp_kldiv keeps
the log-sum-exp form there (tests/test_gpu_vptools.py compares it with the device's own vbmc_vp_pdf for that reason), so on that case
kl_mat follows kldiv_terms and its distance from vbmc_vp_kldiv is recorded, not bounded.  Everywhere else the two are equal."""
import math

import numpy as np
import pytest

from tests import _diag_ref as R
from tests import _mtv_ref as M
from tests import _vptools_ref as T

pytestmark = pytest.mark.gpu
TSTAR_TOL = 4.9e-14        # measured: 4.82e-15 (D5)
DENS_TOL = 1.5e-13         # measured: 1.41e-14 (A2mesh16k, n = 16384; 1.10e-14 at n = 8192, 4.2e-15 at n = 256)
MTV_TOL = 3.2e-14          # measured: 3.11e-15 (G3big)
KL_TOL = 1e-10             # the project's: |dev - ref| <= 1e-10 max(1, |ref|)
ANALYTIC_BOUND = 2.2e-2    # section 6i
SEED = M.SEED
INF = np.inf


def _bounds_runs():
    vp = T.make_vp(2, 3, [3, 1], False, seed=5)
    return [vp, M._other_bounds(T.sibling(vp)), T.sibling(vp, seed=3)]


def _floor_all_runs():
    vp = T.make_case(T.NARROW["case"], width=T.NARROW["width"])
    far = dict(vp)
    far["mu"] = np.asarray(vp["mu"]) + 3.0
    return [vp, far]


def _degenerate_runs():
    vp = M.make_degenerate()
    return [vp, T.sibling(vp)]


CASES = {   # name: (runs, Ns, nkde, nquad)
    "A2": (lambda: R.runs("A", 2), 65, 256, 2),                          # the smallest
    "G3": (lambda: R.runs("G", 3), 1003, 256, 1000),                     # 15 columns
    "B4": (lambda: R.runs("B", 4), 1003, 256, 1000),                     # 16 columns
    "A17": (lambda: R.runs("A", 17), 1003, 256, 1000),                   # 17 columns
    "A17s": (lambda: R.runs("A", 17), 63, 256, 1000),
    "J3": (lambda: R.runs("J", 3), 1003, 256, 1000),                     # D = 13: 39 columns
    "E2": (lambda: R.runs("E", 2, width=2.0), 1003, 256, 1000),          # 64 columns
    "D5": (lambda: R.runs("D", 5), 4097, 8192, 1000),                    # 50 columns on the default mesh
    "G3big": (lambda: R.runs("G", 3), 1003, 8192, 1000),
    "A2mesh16k": (lambda: R.runs("A", 2), 1003, 16384, 1000),            # the cosine table takes 128 KB + 8 of LDS
    "narrow": (lambda: R.runs(T.NARROW["case"], 3, width=T.NARROW["width"]), 1003, 256, 1000),   # vbmc_kldiv.m:76 acts
    "floor_all": (_floor_all_runs, 1003, 256, 1000),                     # ... on every draw of both directions
    "bounds": (_bounds_runs, 1003, 256, 1000),                           # runs with different bounds
    "degenerate": (_degenerate_runs, 1003, 256, 1000),                   # NaN in one dimension
}


@pytest.fixture(scope="module")
def V():
    from vbmc_amd import vptools

    return vptools


_cache = {}


def ran(V, name):
    """The device's call on a case (computed once, never changed)"""
    if name not in _cache:
        make, Ns, nkde, nquad = CASES[name]
        vps = make()
        out = V.vp_diagnostics(vps, Ns, seed=SEED, nkde=nkde, nquad=nquad, stages=True, draws=True)
        for a in out.values():
            a.setflags(write=False)
        _cache[name] = (vps, out)
    return _cache[name]


def unique_rule(vps, xx):
    """(R, D): the clamp-end count with each run's own clamp ends; asserted equal to np.unique"""
    D = xx.shape[2]
    nu = np.zeros((len(vps), D), dtype=np.int64)
    for i, vp in enumerate(vps):
        lb, ub = M.bounds_of(vp, D)
        for d in range(D):
            nu[i, d] = M.clamp_rule(xx[i][:, d], lb[d], ub[d])
            assert nu[i, d] == np.unique(xx[i][:, d]).size, (i, d)
    return nu


@pytest.mark.parametrize("name", [k for k in CASES if k != "degenerate"])
def test_against_the_restatements(V, name):
    _, Ns, nkde, nquad = CASES[name]
    vps, out = ran(V, name)
    nR, D = len(vps), int(vps[0]["D"])
    xx = out["xx"]
    for i, vp in enumerate(vps):
        assert np.array_equal(xx[i], V.vbmc_rnd(vp, Ns, True, True, seed=SEED + i, nargout=1)), i
    nu = unique_rule(vps, xx)
    assert np.array_equal(out["nuniq"], nu)
    assert np.all(out["counts"].sum(axis=2) == Ns)
    inf = np.full(D, INF)
    et = ed = em = ek = 0.0
    share = np.zeros((nR, nR))
    for i in range(nR):
        for j in range(i + 1, nR):
            rmtv, rst = M.mtv(xx[i], xx[j], -inf, inf, -inf, inf, nkde=nkde, nquad=nquad, nuniq=nu[[i, j]])   # (NoBracket: fminbnd)
            for p, r in enumerate((i, j)):
                assert np.array_equal(out["mesh"][r], rst["mesh"][p]), (r, out["mesh"][r], rst["mesh"][p])
                assert np.array_equal(out["counts"][r], rst["counts"][p]), (r, np.argwhere(out["counts"][r] != rst["counts"][p])[:5])
                et = max(et, float(np.max(np.abs(out["tstar"][r] - rst["tstar"][p]) / np.abs(rst["tstar"][p]))))
                ed = max(ed, float(np.max(np.abs(out["density"][r] - rst["density"][p]) / np.max(rst["density"][p], axis=1, keepdims=True))))
            em = max(em, float(np.max(np.abs(out["mtv"][i, j] - rmtv))))
            assert np.array_equal(out["mtv"][i, j], out["mtv"][j, i])
            assert out["maxmtv_mat"][i, j] == np.max(out["mtv"][i, j]) == out["maxmtv_mat"][j, i]
            kls, sh = T.kldiv_terms(vps[i], vps[j], xx[i], xx[j])
            share[i, j], share[j, i] = sh
            for (a, b), ref in (((i, j), kls[0]), ((j, i), kls[1])):
                ek = max(ek, abs(out["kl_mat"][a, b] - ref) / max(1.0, abs(ref)))
    print("DIAG-MEASURE %s tstar %.3e density %.3e mtv %.3e kl %.3e   floor share min %.3f max %.3f" % (name, et, ed, em, ek, share.min(), share.max()))
    assert np.all(np.diag(out["kl_mat"]) == 0) and np.all(np.diag(out["maxmtv_mat"]) == 0) and np.all(out["mtv"][np.arange(nR), np.arange(nR)] == 0)
    assert np.all(out["kl_mat"] >= 0) and np.all(out["mtv"] >= 0)
    assert et <= TSTAR_TOL, (name, et)
    assert ed <= DENS_TOL, (name, ed)
    assert em <= MTV_TOL, (name, em)
    off = share[~np.eye(nR, dtype=bool)]
    if name == "narrow":      # the rule of vbmc_kldiv.m:76 replaces a part of a direction's densities
        assert np.any((off > 0) & (off < 1)), share
    if name == "floor_all":   # and all of them
        assert np.all(off == 1.0), share
    if name == "bounds":
        b = [M.bounds_of(v, D) for v in vps]
        assert np.any(b[0][0] != b[1][0]) and np.array_equal(b[0][0], b[2][0])
    assert ek <= KL_TOL, (name, ek)

def test_kl_against_the_pairwise_call(V):
    """kl_mat[i, j] is what vbmc_vp_kldiv(vp_i, vp_j, Ns, seed + i) returns in kls[0]; two runs are one existing call.  Recorded, not
    bounded, where densities lie below realmin (the module's docstring)."""
    worst = {}
    for name in ("B4", "G3", "narrow"):
        _, Ns, _, _ = CASES[name]
        vps, out = ran(V, name)
        worst[name] = 0.0
        for i in range(len(vps)):
            for j in range(len(vps)):
                if i != j:
                    ref = V.vbmc_kldiv(vps[i], vps[j], Ns, seed=SEED + i)[0]
                    worst[name] = max(worst[name], abs(out["kl_mat"][i, j] - ref) / max(1.0, abs(ref)))
    vps = R.runs("D", 2)
    two = V.vp_diagnostics(vps, 1003, seed=SEED, nkde=256, nquad=1000)
    ref = V.vbmc_kldiv(vps[0], vps[1], 1003, seed=SEED)
    dev2 = float(np.max(np.abs(np.array([two["kl_mat"][0, 1], two["kl_mat"][1, 0]]) - ref) / np.maximum(1.0, np.abs(ref))))
    print("DIAG-MEASURE kl_mat against vbmc_vp_kldiv: worst relative deviation %s, %.3e (two runs of D)" % (worst, dev2))
    assert worst["B4"] <= KL_TOL and worst["G3"] <= KL_TOL and dev2 <= KL_TOL


def test_two_runs_without_a_trinfo_are_vbmc_mtv(V):
    """The draws and the bounds are vbmc_vp_mtv's; the cosine transform is another kernel: within the measured bounds"""
    g0, g1 = M._gauss(2, 0.0, 1.0), M._gauss(2, 0.5, 1.3)
    out = V.vp_diagnostics([g0, g1], 1003, seed=SEED, nkde=256, nquad=1000, stages=True, draws=True)
    mtv, xx1, xx2, st = V.vbmc_mtv(g0, g1, 1003, seed=SEED, nkde=256, nquad=1000, nargout=3, stages=True)
    assert np.array_equal(out["xx"][0], xx1) and np.array_equal(out["xx"][1], xx2)
    for k in ("mesh", "counts", "nuniq"):
        assert np.array_equal(out[k], st[k]), k
    et = float(np.max(np.abs(out["tstar"] - st["tstar"]) / np.abs(st["tstar"])))
    ed = float(np.max(np.abs(out["density"] - st["density"]) / np.max(st["density"], axis=2, keepdims=True)))
    em = float(np.max(np.abs(out["mtv"][0, 1] - mtv)))
    print("DIAG-MEASURE two runs against vbmc_vp_mtv: tstar %.3e density %.3e mtv %.3e" % (et, ed, em))
    assert et <= TSTAR_TOL and ed <= DENS_TOL and em <= MTV_TOL, (et, ed, em)
    assert np.array_equal(out["mtv"][1, 0], out["mtv"][0, 1]) and out["maxmtv_mat"][0, 1] == np.max(out["mtv"][0, 1])


@pytest.mark.parametrize("C,n", [(1, 256), (17, 256), (33, 512)])
def test_cosine_transform_against_the_direct_sums(V, C, n):
    """k_diag_dct (vbmc_test_dct, kernel 1) against the sums dct1d / idct1d stand for and against k_mtv_dct (kernel 0) on the same
    columns, at column counts on both sides of the 16- and 32-column tiles; a column does not depend on its neighbours"""
    import ctypes

    from vbmc_amd import default_engine
    from vbmc_amd._lib import ptr

    ctx = default_engine().ctx
    x = np.random.default_rng(C).random((C, n))
    x /= x.sum(axis=1, keepdims=True)

    def run(kernel, inverse, data):
        out, a2 = np.zeros_like(data), np.zeros_like(data)
        ctx.check(ctx.lib.vbmc_test_dct(ctx.h, n, data.shape[0], inverse, kernel, 1, ptr(data), ptr(out), None if inverse else ptr(a2), ctypes.POINTER(ctypes.c_double)()))
        return out, a2

    for inverse, ref in ((0, M.dct_sum), (1, M.idct_sum)):
        new, a2 = run(1, inverse, x)
        old, _ = run(0, inverse, x)
        want = np.stack([ref(c) for c in x])
        scale = np.max(np.abs(want))
        e_ref, e_old = float(np.max(np.abs(new - want)) / scale), float(np.max(np.abs(new - old)) / scale)
        print("DIAG-MEASURE dct C=%d n=%d inverse=%d against the sums %.3e against k_mtv_dct %.3e" % (C, n, inverse, e_ref, e_old))
        assert e_ref <= 1e-10 and e_old <= 1e-10
        if not inverse:
            assert np.array_equal(a2, (0.5 * new) ** 2)
        alone, _ = run(1, inverse, np.ascontiguousarray(x[-1:]))
        assert np.array_equal(alone[0], new[-1])


def test_repeated_and_subset_calls_are_identical(V):
    _, Ns, nkde, nquad = CASES["B4"]
    vps, out = ran(V, "B4")
    again = V.vp_diagnostics(vps, Ns, seed=SEED, nkde=nkde, nquad=nquad, stages=True, draws=True)
    for k in out:
        assert np.array_equal(again[k], out[k], equal_nan=True), k
    plain = V.vp_diagnostics(vps, Ns, seed=SEED, nkde=nkde, nquad=nquad)                           # no stage pointer, no draws
    for k in plain:
        assert np.array_equal(plain[k], out[k]), k
    # run i draws with seed + i: runs (0, 1) as they are, runs (2, 3) as a call of two on seed + 2
    for first in (0, 2):
        sub = V.vp_diagnostics(vps[first:first + 2], Ns, seed=SEED + first, nkde=nkde, nquad=nquad, stages=True, draws=True)
        for k in ("xx", "mesh", "counts", "nuniq", "tstar", "density"):
            assert np.array_equal(sub[k], out[k][first:first + 2]), (first, k)
        for k in ("kl_mat", "maxmtv_mat", "mtv"):
            assert np.array_equal(sub[k], out[k][first:first + 2, first:first + 2]), (first, k)


def test_degenerate_column(V):
    vps, out = ran(V, "degenerate")
    assert np.all(out["xx"][0][:, 1] == 1.0)
    assert np.all(np.isnan(out["mtv"][0, 1, 1])) and np.all(np.isfinite(out["mtv"][0, 1, [0, 2]])) and np.all(out["mtv"][0, 1, [0, 2]] > 0)
    assert np.all(np.isnan(out["tstar"][:, 1])) and np.all(np.isfinite(out["tstar"][:, [0, 2]]))
    assert out["maxmtv_mat"][0, 1] == np.max(out["mtv"][0, 1, [0, 2]]) == out["maxmtv_mat"][1, 0]   # max skips the NaN (vbmc_diagnostics.m:124)
    assert out["maxmtv_mat"][0, 1] == R.nanskip_max(out["mtv"][0, 1].tolist())
    inf = np.full(3, INF)
    rmtv, _ = M.mtv(out["xx"][0], out["xx"][1], -inf, inf, -inf, inf, nkde=256, nquad=1000)
    print("DIAG-MEASURE degenerate mtv %.3e" % np.max(np.abs(out["mtv"][0, 1, [0, 2]] - rmtv[[0, 2]])))
    assert np.max(np.abs(out["mtv"][0, 1, [0, 2]] - rmtv[[0, 2]])) <= MTV_TOL
    one = M._gauss(1, 0.0, 1.0)
    one["lambda"] = np.array([1e-30])
    one["mu"] = np.array([[1.0]])
    alln = V.vp_diagnostics([one, one], 1003, seed=SEED, nkde=256, nquad=1000)
    assert math.isnan(alln["maxmtv_mat"][0, 1]) and math.isnan(alln["maxmtv_mat"][1, 0]) and alln["maxmtv_mat"][0, 0] == 0   # all dimensions NaN


def test_analytic_value(V):
    """Unit Gaussians with means 0, 0.5 and 2 in one call at Ns = 1e5 on the default mesh: every pair within section 6i's bound"""
    means = (0.0, 0.5, 2.0)
    out = V.vp_diagnostics([M._gauss(1, m, 1.0) for m in means], 1e5, seed=11)
    worst = 0.0
    for i in range(3):
        for j in range(3):
            want = math.erf(abs(means[i] - means[j]) / (2 * math.sqrt(2)))
            worst = max(worst, abs(out["mtv"][i, j, 0] - want))
    print("DIAG-MEASURE analytic worst %.3e" % worst)
    assert worst <= ANALYTIC_BOUND, worst


def test_refusals_leave_the_context_usable(V):
    from vbmc_amd import _lib

    g = [M._gauss(1, 0.1 * i, 1.0) for i in range(33)]
    kw = dict(seed=SEED, nkde=256, nquad=1000)
    ok = V.vp_diagnostics(g[:3], 1003, **kw)
    for vps, status in ((g[:1], _lib.VBMC_ERR_INVALID), (g, _lib.VBMC_ERR_UNSUPPORTED), ([g[0], M._gauss(2, 0.0, 1.0)], _lib.VBMC_ERR_INVALID),
                        ([g[0], T.make_vp(1, 513, None, False)], _lib.VBMC_ERR_UNSUPPORTED)):
        with pytest.raises(_lib.VbmcHipError) as e:
            V.vp_diagnostics(vps, 1003, **kw)
        assert e.value.status == status, (len(vps), e.value)
    with pytest.raises(_lib.VbmcUnsupported, match="run 1, dimension 1"):
        V.vp_diagnostics(g[:2], 5, **kw)
    again = V.vp_diagnostics(g[:3], 1003, **kw)                                                   # the next call works
    for k in ok:
        assert np.array_equal(again[k], ok[k]), k
    assert V.vp_diagnostics(g[:32], 1003, **kw)["kl_mat"].shape == (32, 32)                         # the largest R


def test_end_to_end(V):
    """vbmc_diagnostics on three runs: two posteriors close to each other and one far give PASS; far from both of two others gives -1"""
    vp = T.make_case("B")
    near = dict(vp)
    near["sigma"] = np.ravel(vp["sigma"]) * 1.05
    far = dict(vp)
    far["mu"] = np.asarray(vp["mu"]) + 3.0
    kw = dict(Ns=20000, seed=SEED, nkde=256, nquad=1000, verbose=False)
    runs = [R.with_stats(vp, -1.0), R.with_stats(near, -1.1), R.with_stats(far, -1.3)]
    exitflag, best, idx, stats = V.vbmc_diagnostics(runs, **kw)
    print("DIAG-MEASURE end to end: sKL_best %s maxmtv_best %s" % (np.array2string(stats["sKL_best"], precision=3), np.array2string(stats["maxmtv_best"], precision=3)))
    assert exitflag == 1 and idx == 0 and best["vp"] is runs[0] and best["elbo"] == -1.0
    assert stats["sKL_best"][1] < 1 < stats["sKL_best"][2] and stats["maxmtv_best"][1] < 0.2 < stats["maxmtv_best"][2]
    want = R.decision(stats["elbo"].tolist(), stats["elbo_sd"].tolist(), [True] * 3, stats["kl_mat"].tolist(), stats["maxmtv_mat"].tolist())
    assert want["exitflag"] == 1 and want["best_run"] == 0
    # the far run is the best: nothing agrees with it
    runs[2]["stats"]["elbo"] = -0.5
    exitflag, best, idx, stats2 = V.vbmc_diagnostics(runs, **kw)
    assert exitflag == -1 and idx == 2 and np.array_equal(stats2["kl_mat"], stats["kl_mat"]) and np.array_equal(stats2["maxmtv_mat"], stats["maxmtv_mat"])
    # a given threshold is used, the last one too
    assert V.vbmc_diagnostics(runs, 3, 1, 1e6, 1.5, **kw)[0] == 1
    assert V.vbmc_diagnostics(runs, 3, 1, 1e6, **kw)[0] == -1
    # the same posterior twice: zero total variation only where the draws coincide; the divergences are small
    twice = [R.with_stats(vp, -1.0), R.with_stats(vp, -1.0)]
    exitflag, _, _, s = V.vbmc_diagnostics(twice, **kw)
    assert exitflag == 1 and np.all(s["kl_mat"] < 0.1) and np.all(s["maxmtv_mat"] < 0.2)

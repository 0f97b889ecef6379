"""GPU: vbmc_vp_mtv (vbmc_amd.vptools.vbmc_mtv) stage by stage against the restatement tests/_mtv_ref.py fed the device's own draws,
on the cases of tests/_mtv_ref.make_pair (tests/test_mtv_restatement.py asserts what they rely on: one root per bracket, the unique
count, no zero range).

Identical: xx1 / xx2 against vbmc_vp_rnd's rows, mesh, counts, nuniq, a repeated call, a replayed block, a call without stage
pointers, and mtv == 0 where xx1 and xx2 hold the same samples.
Tolerances.  They were not fixed in advance: each is ten times the largest deviation measured over the cases (DESIGN.md section 6i
lists the measurements) and sits below the project's 1e-10 for values.
  tstar    |dev - ref| <= TSTAR_TOL |ref|
  density  |dev - ref| <= DENS_TOL max(ref)
  mtv      |dev - ref| <= MTV_TOL
The analytic pair (tests/test_mtv_restatement.py) through the device at Ns = 1e5 holds that file's margin, 3 ANALYTIC_WORST."""
import numpy as np
import pytest

from tests import _mtv_ref as M
from tests.test_mtv_restatement import ANALYTIC_MEANS, ANALYTIC_SEEDS, ANALYTIC_WORST, analytic

pytestmark = pytest.mark.gpu
TSTAR_TOL = 3.9e-14        # measured: 3.90e-15 (wide13; the piled column of `pile`, t* = 1.6e-9: 1.78e-15)
DENS_TOL = 7.4e-14         # measured: 7.38e-15 (mixed, n = 8192; 4.55e-15 at n = 16384)
MTV_TOL = 2.3e-14          # measured: 2.26e-15 (mixed, nquad = 100000); 0 exactly on `identical`
SEED = M.SEED


@pytest.fixture(scope="module")
def V():
    from vbmc_amd import vptools

    return vptools


_cache = {}


def blocks(V, name):
    vp1, vp2, Ns, nkde, nquad, same = M.make_pair(name)
    if not same:
        return None, None
    B, _ = V.vp_rnd_rng_dump(SEED, Ns, vp1["D"], vp1["w"], True)
    return B, B


def ran(V, name):
    """The device's call on a case and the restatement on its draws (computed once, never changed)"""
    if name not in _cache:
        vp1, vp2, Ns, nkde, nquad, same = M.make_pair(name)
        b1, b2 = blocks(V, name)
        mtv, xx1, xx2, st = V.vbmc_mtv(vp1, vp2, Ns, seed=SEED, block1=b1, block2=b2, nkde=nkde, nquad=nquad, nargout=3, stages=True)
        D = vp1["D"]
        rmtv, rst = M.mtv(xx1, xx2, *M.bounds_of(vp1, D), *M.bounds_of(vp2, D), nkde=nkde, nquad=nquad)
        for a in (mtv, xx1, xx2, rmtv) + tuple(st.values()):
            a.setflags(write=False)
        _cache[name] = (mtv, xx1, xx2, st, rmtv, rst)
    return _cache[name]


@pytest.mark.parametrize("name", M.PAIRS)
def test_stages_against_the_restatement(V, name):
    vp1, vp2, Ns, nkde, nquad, same = M.make_pair(name)
    mtv, xx1, xx2, st, rmtv, rst = ran(V, name)
    b1, b2 = blocks(V, name)
    assert np.array_equal(xx1, V.vbmc_rnd(vp1, Ns, True, True, seed=SEED, block=b1, nargout=1))
    assert np.array_equal(xx2, V.vbmc_rnd(vp2, Ns, True, True, seed=SEED + 1, block=b2, nargout=1))
    assert np.array_equal(st["mesh"], rst["mesh"]), (st["mesh"], rst["mesh"])
    assert np.array_equal(st["counts"], rst["counts"]), np.argwhere(st["counts"] != rst["counts"])[:5]
    assert np.all(st["counts"].sum(axis=2) == Ns)
    assert np.array_equal(st["nuniq"], rst["nuniq"]), (st["nuniq"], rst["nuniq"])
    et = float(np.max(np.abs(st["tstar"] - rst["tstar"]) / np.abs(rst["tstar"])))
    ed = float(np.max(np.abs(st["density"] - rst["density"]) / np.max(rst["density"], axis=2, keepdims=True)))
    em = float(np.max(np.abs(mtv - rmtv)))
    print("MTV-MEASURE %s tstar %.3e density %.3e mtv %.3e   (mtv %s)" % (name, et, ed, em, np.array2string(rmtv, precision=4)))
    assert et <= TSTAR_TOL, (name, et)
    assert ed <= DENS_TOL, (name, ed)
    assert em <= MTV_TOL, (name, em)
    assert np.all(mtv >= 0)


def test_mesh_arrangements(V):
    assert np.all(ran(V, "identical")[0] == 0.0)                                      # the same samples: |s1 - s2| is exactly zero
    assert np.array_equal(np.sort(ran(V, "identical")[1], axis=0), np.sort(ran(V, "identical")[2], axis=0))
    m = ran(V, "disjoint")
    lo = m[3]["mesh"][:, 0, 0]
    hi = m[3]["mesh"][:, 0, 1]
    assert hi[0] < lo[1] and abs(m[0][0] - 1.0) <= 1e-3, (lo, hi, m[0])               # each density has the trapezoid sum one on its own 256 mesh points
    n = ran(V, "nested")[3]["mesh"]
    assert n[0, 0, 0] < n[1, 0, 0] and n[1, 0, 1] < n[0, 0, 1]
    o = ran(V, "empty")[3]["mesh"]
    assert o[0, 0, 0] < o[1, 0, 0] < o[0, 0, 1] < o[1, 0, 1]
    b = ran(V, "bounds")[3]["mesh"]
    assert np.all(b[0] != b[1])


def test_pile_on_the_clamp_ends(V):
    _, xx1, _, st, _, _ = ran(V, "pile")
    assert st["nuniq"][0, 0] < xx1.shape[0] and st["nuniq"][0, 1] == xx1.shape[0]
    assert 0 < st["tstar"][0, 0] < 1e-6


def test_repeated_calls_are_identical(V):
    name = "mixed"
    vp1, vp2, Ns, nkde, nquad, _ = M.make_pair(name)
    mtv, xx1, xx2, st, _, _ = ran(V, name)
    again = V.vbmc_mtv(vp1, vp2, Ns, seed=SEED, nkde=nkde, nquad=nquad, nargout=3, stages=True)
    assert np.array_equal(again[0], mtv) and np.array_equal(again[1], xx1) and np.array_equal(again[2], xx2)
    for k in st:
        assert np.array_equal(again[3][k], st[k]), k
    B1, _ = V.vp_rnd_rng_dump(SEED, Ns, vp1["D"], vp1["w"], True)
    B2, _ = V.vp_rnd_rng_dump(SEED + 1, Ns, vp2["D"], vp2["w"], True)
    replay = V.vbmc_mtv(vp1, vp2, Ns, seed=SEED, block1=B1, block2=B2, nkde=nkde, nquad=nquad, nargout=3)
    assert np.array_equal(replay[0], mtv) and np.array_equal(replay[1], xx1) and np.array_equal(replay[2], xx2)
    assert np.array_equal(V.vbmc_mtv(vp1, vp2, Ns, seed=SEED, nkde=nkde, nquad=nquad), mtv)   # no stage pointer, no xx1 / xx2


def test_refusals_leave_the_context_usable(V):
    from vbmc_amd import _lib

    g0, g1 = M._gauss(1, 0.0, 1.0), M._gauss(1, 0.5, 1.0)
    with pytest.raises(_lib.VbmcUnsupported, match="posterior 1, dimension 1"):
        V.vbmc_mtv(g0, g1, 5, seed=SEED, nkde=256, nquad=1000)
    ok = V.vbmc_mtv(g0, g1, 1003, seed=SEED, nkde=256, nquad=1000)
    assert np.isfinite(ok[0]) and 0 < ok[0] < 1
    for kw, vps in ((dict(Ns=1003, nkde=256), (g0, M._gauss(2, 0.0, 1.0))), (dict(Ns=1003, nkde=300), (g0, g1)), (dict(Ns=1, nkde=256), (g0, g1))):
        with pytest.raises(_lib.VbmcHipError) as e:
            V.vbmc_mtv(vps[0], vps[1], kw["Ns"], seed=SEED, nkde=kw["nkde"], nquad=1000)
        assert e.value.status == _lib.VBMC_ERR_INVALID, (kw, e.value)
    assert np.array_equal(V.vbmc_mtv(g0, g1, 1003, seed=SEED, nkde=256, nquad=1000), ok)


def test_degenerate_column(V):
    vp = M.make_degenerate()
    mtv, xx1, xx2, st = V.vbmc_mtv(vp, vp, 1003, seed=SEED, nkde=256, nquad=1000, nargout=3, stages=True)
    assert np.all(xx1[:, 1] == 1.0) and np.all(xx2[:, 1] == 1.0)
    assert np.isnan(mtv[1]) and np.all(np.isfinite(mtv[[0, 2]])) and np.all(mtv[[0, 2]] > 0)
    assert np.all(np.isnan(st["tstar"][:, 1])) and np.all(np.isfinite(st["tstar"][:, [0, 2]]))
    rmtv, _ = M.mtv(xx1, xx2, *M.bounds_of(vp, 3), *M.bounds_of(vp, 3), nkde=256, nquad=1000)
    print("MTV-MEASURE degenerate mtv %.3e" % np.max(np.abs(mtv[[0, 2]] - rmtv[[0, 2]])))
    assert np.max(np.abs(mtv[[0, 2]] - rmtv[[0, 2]])) <= MTV_TOL


@pytest.mark.parametrize("m", ANALYTIC_MEANS)
def test_analytic_pair(V, m):
    worst = 0.0
    for seed in ANALYTIC_SEEDS:
        got = V.vbmc_mtv(M._gauss(1, 0.0, 1.0), M._gauss(1, m, 1.0), 1e5, seed=seed)
        worst = max(worst, abs(got[0] - analytic(m)))
    print("MTV-MEASURE analytic through the device m=%g worst %.3e" % (m, worst))
    assert worst <= 3 * ANALYTIC_WORST, (m, worst)

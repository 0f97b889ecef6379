"""GPU: vbmc_vp_corner (vbmc_amd.vptools.vbmc_plot_data / cornerplot_data) stage by stage against the restatement
tests/_corner_ref.py fed the device's own samples, on the cases of tests/_corner_ref.make_case (tests/test_corner_restatement.py
asserts what they rely on: a bracket with one root in it).

Identical: xx against vbmc_vp_rnd's rows, bounds, hist, counts2 (whose sum is the number of rows inside the bounds), the order
statistics and quant, a repeated call, a replayed block, a call without stage pointers.
Tolerances.  They were not fixed in advance: each is ten times the largest deviation measured over the cases (DESIGN.md section 6m
lists the measurements) and sits below the project's 1e-10 for values.
  tstar      |dev - ref| <= TSTAR_TOL |ref|
  bandwidth  |dev - ref| <= BW_TOL |ref|
  density    |dev - ref| <= DENS_TOL max(ref) of the pair (the restatement's FFT and the device's direct sums differ in the last bits,
             and where the reference clamps a -1e-17 to eps the device may hold +1e-17: never relative to the value itself)
The analytic anchor (tests/test_corner_restatement.py) through the device at Ns = 1e5 holds that file's margin, 3 ANALYTIC_WORST."""
import numpy as np
import pytest

from tests import _corner_ref as R
from tests.test_corner_restatement import ANALYTIC_SEEDS, ANALYTIC_WORST, analytic_error

pytestmark = pytest.mark.gpu
TSTAR_TOL = 1.9e-14        # measured: 1.887e-15 (pile, t* = 8.6e-5; wide32 over 496 pairs: 1.867e-15)
BW_TOL = 1.2e-14           # measured: 1.156e-15 (cut0)
DENS_TOL = 2.2e-14         # measured: 2.193e-15 (three64; 1.724e-15 on cut0)
SEED = R.SEED
P = R.QUANT_P


@pytest.fixture(scope="module")
def V():
    from vbmc_amd import vptools

    return vptools


_cache = {}


def case_bounds(V, name):
    vp, Ns, res, bounds, bal = R.make_case(name)
    if isinstance(bounds, str):
        bounds = R.cut_bounds(V.vbmc_rnd(vp, Ns, True, bool(bal), seed=SEED, nargout=1))
    return bounds


def ran(V, name):
    """The device's call on a case and the restatement on its samples (computed once, never changed)"""
    if name not in _cache:
        if name == "edge":
            X, b = R.edge_matrix()
            dev = V.cornerplot_data(X, b, res=32, p=P, stages=True)
            res = 32
        else:
            vp, Ns, res, _, bal = R.make_case(name)
            b = case_bounds(V, name)
            dev = V.vbmc_plot_data(vp, Ns, seed=SEED, balanceflag=bal, bounds=b, res=res, p=P, stages=True)
        ref = R.corner(dev["xx"], b, res, 40, P)
        for a in dev.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (dev, ref)
    return _cache[name]


def compare(name, dev, ref):
    assert np.array_equal(dev["bounds"], ref["bounds"]), (dev["bounds"], ref["bounds"])
    assert np.array_equal(dev["hist"], ref["hist"]), np.argwhere(dev["hist"] != ref["hist"])[:5]
    assert np.array_equal(dev["counts2"], ref["counts2"]), np.argwhere(dev["counts2"] != ref["counts2"])[:5]
    assert dev["pairs"] == ref["pairs"]
    xx, b = dev["xx"], dev["bounds"]
    inside = (xx >= b[None, :, 0]) & (xx <= b[None, :, 1])
    assert np.array_equal(dev["hist"].sum(axis=1), inside.sum(axis=0))
    for pp, (d1, d2) in enumerate(dev["pairs"]):
        assert dev["counts2"][pp].sum() == np.sum(inside[:, d1] & inside[:, d2]), (name, pp)
    assert np.array_equal(dev["quant"], ref["quant"]), (dev["quant"], ref["quant"])
    if not dev["pairs"]:
        return 0.0, 0.0, 0.0
    et = float(np.max(np.abs(dev["tstar"] - ref["tstar"]) / np.abs(ref["tstar"])))
    eb = float(np.max(np.abs(dev["bandwidth"] - ref["bandwidth"]) / np.abs(ref["bandwidth"])))
    ed = float(np.max(np.abs(dev["density"] - ref["density"]) / np.max(ref["density"], axis=(1, 2), keepdims=True)))
    return et, eb, ed


@pytest.mark.parametrize("name", R.VP_CASES + ("edge",))
def test_stages_against_the_restatement(V, name):
    dev, ref = ran(V, name)
    if name != "edge":
        vp, Ns, res, _, bal = R.make_case(name)
        assert np.array_equal(dev["xx"], V.vbmc_rnd(vp, Ns, True, bool(bal), seed=SEED, nargout=1))
    else:
        assert np.array_equal(dev["xx"], R.edge_matrix()[0])
    et, eb, ed = compare(name, dev, ref)
    print("CORNER-MEASURE %s tstar %.3e bandwidth %.3e density %.3e   (P = %d, tstar %.3e .. %.3e)"
          % (name, et, eb, ed, len(dev["pairs"]), np.min(ref["tstar"], initial=np.inf), np.max(ref["tstar"], initial=0.0)))
    assert et <= TSTAR_TOL, (name, et)
    assert eb <= BW_TOL, (name, eb)
    assert ed <= DENS_TOL, (name, ed)
    assert np.all(dev["density"] > 0)


def test_order_statistics(V):
    """Every rank the probabilities ask for, and the two ends, as np.sort places them -- on the column with ties too"""
    dev, _ = ran(V, "pile")
    xx = dev["xx"]
    s = np.sort(xx, axis=0)
    n = xx.shape[0]
    assert np.sum(xx[:, 0] == s[0, 0]) > 50 and np.sum(xx[:, 0] == s[-1, 0]) > 50                 # ties on both clamp ends
    for p in ((0.5,), (0.0, 1.0), (0.1, 0.9, 0.5), tuple(np.linspace(0.0, 1.0, 16))):
        got = V.vbmc_plot_data(R.make_case("pile")[0], n, seed=SEED, balanceflag=1, res=32, p=p)["quant"]
        want = np.stack([R.quantile1(xx[:, d], p) for d in range(xx.shape[1])])
        assert np.array_equal(got, want), (p, got, want)
    k, kp1, r = R.quantile_ranks((0.0, 1.0), n)
    q = V.cornerplot_data(xx, p=(0.0, 1.0))["quant"]
    assert np.array_equal(q[:, 0], s[0]) and np.array_equal(q[:, 1], s[-1])
    neg = np.array([[-0.0], [0.0], [-1.5], [np.nextafter(0, -1)], [3.0], [-2.0 ** -1060]])        # signs and subnormals in the key order
    ps = tuple((i + 0.5) / 6 for i in range(6))
    q = V.cornerplot_data(neg, p=ps, res=16)["quant"][0]
    assert np.array_equal(q, R.quantile1(neg[:, 0], ps)) and np.max(np.abs(q - np.sort(neg[:, 0]))) <= 1e-15


def test_pair_order_and_transposition(V):
    """Unequal marginals: pair pp is (d1, d2) in cornerplot's order, rows of the density run over d2's mesh and columns over d1's"""
    dev, ref = ran(V, "three64")
    assert dev["pairs"] == [(0, 1), (0, 2), (1, 2)]
    xx, b, n = dev["xx"], dev["bounds"], 64
    for pp, (d1, d2) in enumerate(dev["pairs"]):
        dens = dev["density"][pp]
        cell = np.prod(b[[d1, d2], 1] - b[[d1, d2], 0]) / (n - 1) ** 2
        assert abs(dens.sum() * cell - 1.0) < 0.05                                                # a density on the mesh of bounds_out
        for d, axis in ((d1, 0), (d2, 1)):                                                        # summing rows out leaves d1's marginal
            mesh = np.linspace(b[d, 0], b[d, 1], n)
            marg = dens.sum(axis=axis)
            assert abs(np.sum(mesh * marg) / marg.sum() - np.mean(xx[:, d])) < 0.05 * (b[d, 1] - b[d, 0]), (pp, d)
        assert np.array_equal(dev["counts2"][pp].sum(axis=1), np.bincount(R.ndhist_bins((xx[:, d1] - b[d1, 0]) / (b[d1, 1] - b[d1, 0]), n) - 1, minlength=n))


def test_repeated_calls_are_identical(V):
    name = "cut1"
    vp, Ns, res, _, bal = R.make_case(name)
    b = case_bounds(V, name)
    dev, _ = ran(V, name)
    kw = dict(seed=SEED, balanceflag=bal, bounds=b, res=res, p=P)
    again = V.vbmc_plot_data(vp, Ns, stages=True, **kw)
    for k, v in dev.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(again[k], v), k
    B, _ = V.vp_rnd_rng_dump(SEED, Ns, vp["D"], vp["w"], bool(bal))
    replay = V.vbmc_plot_data(vp, Ns, block=B, **kw)                                              # no stage pointers either
    assert "tstar" not in replay
    for k, v in replay.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(dev[k], v), k
    given = V.cornerplot_data(dev["xx"], b, res=res, p=P, stages=True)                            # the same samples as a given matrix
    for k, v in given.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(dev[k], v), k


def test_balance_flag_reaches_the_draw(V):
    a, b = ran(V, "cut0")[0]["xx"], ran(V, "cut1")[0]["xx"]
    assert a.shape == b.shape and not np.array_equal(a, b)


def test_refusals_leave_the_context_usable(V):
    from vbmc_amd import _lib

    vp, Ns, res, _, bal = R.make_case("small")
    ok = V.vbmc_plot_data(vp, Ns, seed=SEED, res=res)
    X, b = R.edge_matrix()
    bad_b = b.copy()
    bad_b[1] = [1.0, 1.0]
    Xn = X.copy()
    Xn[17, 1] = np.nan
    Xi = X.copy()
    Xi[5, 0] = np.inf
    invalid = (lambda: V.vbmc_plot_data(vp, 1, seed=SEED, res=res), lambda: V.cornerplot_data(X, bad_b, res=32),
               lambda: V.cornerplot_data(Xn, b, res=32), lambda: V.cornerplot_data(Xi, None, res=32),
               lambda: V.cornerplot_data(X, b, res=32, p=(1.5,)), lambda: V.cornerplot_data(X, b, res=32, nbins=2000))
    for call in invalid:
        with pytest.raises(_lib.VbmcHipError) as e:
            call()
        assert e.value.status == _lib.VBMC_ERR_INVALID, e.value
    with pytest.raises(_lib.VbmcUnsupported, match="res = 128"):
        V.vbmc_plot_data(vp, Ns, seed=SEED, res=128)
    Xs, bs = R.small_cut()
    with pytest.raises(R.NoBracket):
        R.corner(Xs, bs, 64, 40, ())
    with pytest.raises(_lib.VbmcUnsupported, match="pair 1, dimensions 1 and 2"):
        V.cornerplot_data(Xs, bs, res=64)
    again = V.vbmc_plot_data(vp, Ns, seed=SEED, res=res)
    for k, v in ok.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(again[k], v), k


def test_zero_range_column(V):
    from tests import _mtv_ref

    vp = _mtv_ref.make_degenerate()
    dev = V.vbmc_plot_data(vp, 1003, seed=SEED, res=32, p=P, stages=True)
    assert np.all(dev["xx"][:, 1] == 1.0)
    ref = R.corner(dev["xx"], None, 32, 40, P)
    assert dev["pairs"] == [(0, 1), (0, 2), (1, 2)]
    for k in ("density", "bandwidth", "tstar"):
        nan = np.isnan(dev[k].reshape(3, -1))
        assert np.all(nan[[0, 2]]) and not np.any(nan[1]), k                                      # NaN in exactly the pairs that hold the column
    assert np.all(dev["hist"][1] == 0) and np.all(dev["hist"][[0, 2]].sum(axis=1) == 1003)
    assert np.array_equal(dev["hist"], ref["hist"]) and np.array_equal(dev["quant"], ref["quant"]) and np.array_equal(dev["bounds"], ref["bounds"])
    assert np.array_equal(dev["counts2"], ref["counts2"])
    et = abs(dev["tstar"][1] - ref["tstar"][1]) / ref["tstar"][1]
    ed = np.max(np.abs(dev["density"][1] - ref["density"][1])) / np.max(ref["density"][1])
    print("CORNER-MEASURE degenerate tstar %.3e density %.3e" % (et, ed))
    assert et <= TSTAR_TOL and ed <= DENS_TOL


def test_analytic_anchor(V):
    vp = dict(D=2, K=1, mu=np.zeros((2, 1)), sigma=np.ones(1), w=np.ones(1), trinfo=None)
    vp["lambda"] = np.ones(2)
    worst = 0.0
    for seed in ANALYTIC_SEEDS:
        dev = V.vbmc_plot_data(vp, 1e5, seed=seed, res=64, p=())
        worst = max(worst, analytic_error(dev["xx"], dev["density"][0], dev["bounds"]))
    print("CORNER-MEASURE analytic through the device worst %.4e" % worst)
    assert worst <= 3 * ANALYTIC_WORST, worst

"""GPU: the variational-posterior tools (vbmc_amd.vptools) where tests/test_gpu_vptools.py does not go.  That file's parametrised tests
run cases A .. O of tests/_vptools_ref.py -- every padded width and a chunk seam at every width from 8 on --; this one holds

  the device to the 50-digit values of tests/golden/mp_vptools_case{0..5}.json directly, at 1e-12 (restatement against 50 digits,
      tests/test_vptools_restatement.py) plus the tolerance of tests/test_gpu_vptools.py (device against restatement), in the units of
      that file's close() and of the gradient check;
  the underflow band to the 50-digit values of mp_vptools_band.json and to the rule of DESIGN.md section 6h: above log(5e-324) of the
      transformed-space mixture the log density is an ordinary number, below it -Inf resp. 0;
  the transform's edges to the restatement, NaN included: subnormal distances from a bound, logit arguments next to 0 and 1, log-Jacobian
      arguments up to 1e4, coordinates whose square overflows, points on and beyond a bound (NaN in both forms, never +Inf), the clamp
      ends of the inverse transform;
  a NaN input coordinate (NaN out) and an infinite one (-Inf resp. 0 out), zero-weight components, a bad row's neighbours (bit-identical), and the refusal of K = 513.

Nothing here leaves a row of its inputs out.  Tolerances are those of tests/test_gpu_vptools.py, unchanged."""
import json
import os

import numpy as np
import pytest

from tests import _vptools_ref as T
from tests.test_gpu_vptools import GRAD_TOL, PDF_TOL, SEED, XORIG_TOL, check_kldiv, check_moments

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = 1e-12                     # tests/test_vptools_restatement.py: the restatement against the 50-digit values
STEP = 4.95e-324                 # one subnormal step (the final ldexp into the subnormal range)
FAMILIES = (("gauss", np.inf), ("mvt", 5.0), ("unit", -5.0))


@pytest.fixture(scope="module")
def V():
    from vbmc_amd import vptools

    return vptools


def load(i):
    """as tests/test_vptools_restatement.py::load"""
    with open(os.path.join(ROOT, "tests", "golden", "mp_vptools_case%d.json" % i)) as f:
        g = json.load(f)
    vp = dict(g["vp"], trinfo=g["trinfo"])
    vp["mu"] = np.array(vp["mu"])
    return g, vp


def same(dev, ref, tol, what, plain=False):
    """Non-finite entries (NaN included) and zeros of a plain density identical; the others within tol of max(1, |ref|), a plain
    density relative to ref.  Every row takes part."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    exact = ~np.isfinite(ref) | ((ref == 0) if plain else False)
    assert np.array_equal(dev[exact], ref[exact], equal_nan=True), (what, dev[exact], ref[exact])
    assert not np.any(np.isposinf(dev) & ~np.isposinf(ref)), (what, dev)
    ok = ~exact
    with np.errstate(all="ignore"):
        err = float(np.max(np.abs(dev[ok] - ref[ok]) / (np.abs(ref[ok]) if plain else np.maximum(1.0, np.abs(ref[ok]))))) if ok.any() else 0.0
    print("VPT-MEASURE edges %s %.3e" % (what, err))
    assert err <= tol, (what, err, dev, ref)


# ---------------------------------------------------------------------------------------------------------------- 50 digits
@pytest.mark.parametrize("i", range(6))
def test_device_against_the_50_digit_fixtures(V, i):
    g, vp = load(i)
    X, Y, tr = np.array(g["X"]), np.array(g["Y"]), g["trinfo"]
    tol = GOLD + PDF_TOL["gauss"]
    lj = np.array(g["logjac"])
    same(V.vbmc_pdf(vp, X, True, True), g["logpdf_orig"], tol, "case%d log pdf orig" % i)
    same(V.vbmc_pdf(vp, X, True, False), g["pdf_orig"], tol, "case%d pdf orig" % i, plain=True)
    same(V.vbmc_pdf(vp, Y, False, True), g["logpdf_trans"], tol, "case%d log pdf trans" % i)
    same(V.vbmc_pdf(vp, Y, True, True, True), np.array(g["logpdf_trans"]) - lj, tol, "case%d log pdf transflag" % i)
    # plain values the fixture holds as logarithms: its double of log p carries p to half a spacing of |log p| (<= 2e-15 here)
    same(V.vbmc_pdf(vp, Y, False, False), np.exp(g["logpdf_trans"]), tol, "case%d pdf trans" % i, plain=True)
    same(V.vbmc_pdf(vp, Y, True, False, True), np.exp(np.array(g["logpdf_trans"]) - lj), tol, "case%d pdf transflag" % i, plain=True)
    for df in g["dfs"]:
        fam = "mvt" if df > 0 else "unit"
        h = np.array(g["heavy"][str(df)])
        same(V.vbmc_pdf(vp, X, True, True, False, df), h, GOLD + PDF_TOL[fam], "case%d log pdf %s" % (i, fam))
        same(V.vbmc_pdf(vp, X, True, False, False, df), np.exp(h), GOLD + PDF_TOL[fam], "case%d pdf %s" % (i, fam), plain=True)
    if g["grad"] is not None:
        for logflag, key in ((False, "grad"), (True, "gradlog")):
            ref = np.array(g[key])
            _, dy = V.vbmc_pdf(vp, Y, False, logflag, nargout=2)
            # the device within GRAD_TOL of a row's largest entry of the restatement, which is within 1e-12 of the fixture in the units of
            # its own check: of the row's largest entry (plain) resp. of max(1, |entry|) (log)
            rowmax = np.max(np.abs(ref), axis=1, keepdims=True)
            bound = GRAD_TOL * rowmax + GOLD * (rowmax if not logflag else np.maximum(1.0, np.abs(ref)))
            print("VPT-MEASURE edges case%d %s %.3e of the bound" % (i, key, float(np.max(np.abs(dy - ref) / bound))))
            assert np.all(np.abs(dy - ref) <= bound), (i, key, np.max(np.abs(dy - ref) / bound))
    # vbmc_rnd's inverse transform: a mixture whose components sit at the fixture's Y, a block of zero normals whose uniforms name
    # component i for row i: the transformed-space sample is Y exactly, the output its inverse
    N, D = Y.shape
    vq = dict(D=D, K=N, mu=Y.T.copy(), sigma=np.ones(N), w=np.full(N, 1.0 / N), trinfo=tr)
    vq["lambda"] = np.ones(D)
    B = np.zeros((N, D + 1))
    B[:, 0] = (np.arange(N) + 0.5) / N
    Xd, Id = V.vbmc_rnd(vq, N, True, False, seed=SEED, block=B)
    assert np.array_equal(Id, np.arange(N))
    assert np.array_equal(V.vbmc_rnd(vq, N, False, False, seed=SEED, block=B)[0], Y)
    same(Xd, g["inverse"], GOLD + XORIG_TOL, "case%d inverse through vbmc_rnd" % i)


# ---------------------------------------------------------------------------------------------------------------- the underflow band
@pytest.mark.parametrize("j", range(2))
def test_underflow_band_against_50_digits(V, j):
    with open(os.path.join(ROOT, "tests", "golden", "mp_vptools_band.json")) as f:
        g = json.load(f)
    m, thr = g["mixtures"][j], g["threshold"]
    vp = dict(m["vp"], trinfo=m["trinfo"])
    vp["mu"] = np.array(vp["mu"])
    X = np.array(m["X"])
    above = np.array(m["logmix_trans"]) > thr          # the rule acts on the transformed-space mixture, before the Jacobian
    tol = GOLD + PDF_TOL["gauss"]
    ref_log = np.where(above, np.array(m["logpdf_orig"]), -np.inf)
    ref = np.where(above, np.array(m["pdf_orig"]), 0.0)
    dev_l, dev = V.vbmc_pdf(vp, X, True, True), V.vbmc_pdf(vp, X, True, False)
    print("VPT-MEASURE band %d log %s" % (j, dev_l.tolist()))
    print("VPT-MEASURE band %d plain %s" % (j, dev.tolist()))
    same(dev_l, ref_log, tol, "band %d log pdf" % j)
    assert np.all(dev[~above] == 0.0), dev
    assert np.all(np.abs(dev - ref)[above] <= (PDF_TOL["gauss"] * ref + STEP)[above]), (dev, ref)
    for df in g["dfs"]:
        fam = "mvt" if df > 0 else "unit"
        h = np.array(m["heavy"][str(df)])
        assert np.all(np.isfinite(h)) and np.all(h > thr)
        same(V.vbmc_pdf(vp, X, True, True, False, df), h, GOLD + PDF_TOL[fam], "band %d log pdf %s" % (j, fam))
        assert np.all(np.abs(V.vbmc_pdf(vp, X, True, False, False, df) - np.exp(h)) <= (GOLD + PDF_TOL[fam]) * np.exp(h) + STEP)


# ---------------------------------------------------------------------------------------------------------------- the transform's edges
def pdf_all(V, vp, X, what, transflag=False):
    """Every family, log and plain, against the restatement with NaN and +-Inf compared exactly"""
    for fam, df in FAMILIES:
        for logflag in (True, False):
            same(V.vbmc_pdf(vp, X, True, logflag, transflag, df), T.pdf(vp, X, True, logflag, transflag, df), PDF_TOL[fam],
                 "%s %s log=%d" % (what, fam, logflag), plain=not logflag)


@pytest.mark.parametrize("which", ["zero_bounds", "logit"])
def test_rows_next_to_on_and_beyond_a_bound(V, which):
    vp, rows = (T.make_zero_bounds(), T.zero_bounds_rows()) if which == "zero_bounds" else (T.make_logit(), T.logit_rows())
    for X, tag in zip(rows, ("near", "huge", "on", "outside")):
        pdf_all(V, vp, X, "%s %s" % (which, tag))
    for X in rows[2:]:                                     # on and beyond a bound: NaN in both forms, never +Inf
        for logflag in (True, False):
            y = V.vbmc_pdf(vp, X, True, logflag)
            assert np.isfinite(y[0]) and np.all(np.isnan(y[1:])), (which, logflag, y)


def test_log_jacobian_far_out(V):
    vp = T.make_logit()
    zs = [s * z for z in T.LOGIT_Z for s in (1.0, -1.0) if s * z > -T.LOGIT_Z_REF_OVERFLOWS]
    pdf_all(V, vp, T.logit_trans_rows(vp, zs), "logit transflag", transflag=True)
    # Past exp's range on the negative side the reference's exp(-z) is Inf and its log-Jacobian -Inf; the device takes the even
    # function -z - 2 log1p(exp(-z)) at |z| and stays finite: held to that closed form
    tr = vp["trinfo"]
    Yt = T.logit_trans_rows(vp, [-z for z in T.LOGIT_Z if z > T.LOGIT_Z_REF_OVERFLOWS])
    az = np.abs(Yt[:, 0] * tr["delta"][0] + tr["mu"][0])
    lj = np.log(tr["ub_orig"][0] - tr["lb_orig"][0]) + (-az - 2 * np.log1p(np.exp(-az))) + np.log(tr["delta"][0]) + np.log(tr["delta"][1])
    for logflag in (True, False):
        ref = T.pdf(vp, Yt, False, True) - lj               # (the plain density as the device forms it: exp(log p - log J))
        ref = ref if logflag else np.exp(ref)
        same(V.vbmc_pdf(vp, Yt, True, logflag, True), ref, PDF_TOL["gauss"], "logit transflag, even log-Jacobian log=%d" % logflag, plain=not logflag)


def test_a_nan_coordinate_stays_nan(V):
    """A NaN in the input is NaN in the result, in every family and both forms, with and without a transform (the table exponential's
    lower clamp drops a NaN: unguarded, such a row came out as -Inf resp. 0)"""
    for vp in (T.make_case("G"), T.make_vp(2, 3, None, False), T.make_zero_bounds()):
        D = int(vp["D"])
        Y = np.asarray(vp["mu"]).T[[0] * (D + 1)] + 0.1
        X = T.warp(Y, "i", vp["trinfo"])
        for d in range(D):
            X[d + 1, d], Y[d + 1, d] = np.nan, np.nan
        pdf_all(V, vp, X, "nan D=%d" % D)
        for fam, df in FAMILIES:
            for logflag in (True, False):
                y = V.vbmc_pdf(vp, Y, False, logflag, False, df)
                same(y, T.pdf(vp, Y, False, logflag, False, df), PDF_TOL[fam], "nan trans D=%d %s log=%d" % (D, fam, logflag), plain=not logflag)
                assert np.isfinite(y[0]) and np.all(np.isnan(y[1:])), (D, fam, logflag, y)
        for logflag in (True, False):
            y, dy = V.vbmc_pdf(vp, Y, False, logflag, nargout=2)
            assert np.all(np.isnan(y[1:])) and np.all(np.isnan(dy[1:])) and np.all(np.isfinite(dy[0])), (D, logflag, y, dy)


def test_an_infinite_coordinate_is_not_a_nan(V):
    """+-Inf in a coordinate: the squared distance is Inf and the density -Inf resp. 0, not NaN -- also where the rotation's zero
    padding turns the infinity into a NaN of the padded registers (D = 5 of 8 and 13 of 16, type-0 variables: with other types the
    reference's own log-Jacobian un-rotates an infinite vector and is NaN by Inf - Inf), and for log(Inf) of a type-1 / type-2 variable"""
    for D in (5, 13):
        vp = T.make_vp(D, 3, [0] * D, True)
        X = T.warp(np.asarray(vp["mu"]).T[[0] * (2 * D + 1)] + 0.1, "i", vp["trinfo"])
        for d in range(D):
            X[2 * d + 1, d], X[2 * d + 2, d] = np.inf, -np.inf
        pdf_all(V, vp, X, "inf rotated D=%d" % D)
        y = V.vbmc_pdf(vp, X, True, True)
        assert np.isfinite(y[0]) and np.all(np.isneginf(y[1:])), y
    vp = T.make_zero_bounds()
    X = T.zero_bounds_rows()[0][[0] * 5]
    X[1, 0], X[2, 1], X[3, 2], X[4, 2] = np.inf, -np.inf, np.inf, -np.inf
    pdf_all(V, vp, X, "inf zero_bounds")
    y = V.vbmc_pdf(vp, X, True, True)
    assert np.isfinite(y[0]) and np.all(np.isneginf(y[1:])), y


@pytest.mark.parametrize("balanced", [False, True])
def test_inverse_transform_reaches_the_clamp_ends(V, balanced):
    vp = T.make_clamp()
    N = 65
    B, perm = V.vp_rnd_rng_dump(SEED, N, vp["D"], vp["w"], balanced)
    B = T.clamp_block(B, perm)
    X, I, _ = T.rnd(vp, N, True, balanced, B, SEED)
    Xd, Id = V.vbmc_rnd(vp, N, True, balanced, seed=SEED, block=B)
    assert np.array_equal(Id, I)
    same(Xd, X, XORIG_TOL, "clamp bal=%d" % balanced)
    lo, hi = T.clamp_ends(vp["trinfo"])
    rows = [r for r, _ in T.CLAMP_ROWS]
    assert np.array_equal(Xd[rows][:, 1:], X[rows][:, 1:])              # the ends themselves, +Inf and -Inf: exactly
    assert np.any(Xd == lo) and np.any(Xd == hi) and np.any(np.isposinf(Xd[:, 1])) and np.all(Xd >= lo) and np.all(Xd <= hi)


# ---------------------------------------------------------------------------------------------------------------- zero weights
@pytest.mark.parametrize("which", T.ZERO_WEIGHTS)
def test_zero_weight_components(V, which):
    vp = T.make_zero_weight(which)
    tag = "w%s=0" % (list(which),)
    N, dead = 1003, list(which)
    for balanced in (False, True):
        B, _ = V.vp_rnd_rng_dump(SEED, N, vp["D"], vp["w"], balanced)
        X, I, Y = T.rnd(vp, N, True, balanced, B, SEED)
        Xd, Id = V.vbmc_rnd(vp, N, True, balanced, seed=SEED)
        assert np.array_equal(Id, I) and not np.isin(Id, dead).any(), tag
        assert np.array_equal(V.vbmc_rnd(vp, N, False, balanced, seed=SEED)[0], Y), tag
        same(Xd, X, XORIG_TOL, "%s rnd bal=%d" % (tag, balanced))
    X, Y = X[:65], Y[:65]
    far = T.far_point(vp)                                    # every live component's term underflows after the dead ones' -1e300
    pdf_all(V, vp, np.vstack([X, far]), tag + " pdf")
    Yt = np.vstack([Y, T.warp(far, "d", vp["trinfo"])])
    for fam, df in FAMILIES:
        for logflag in (True, False):
            same(V.vbmc_pdf(vp, Yt, False, logflag, False, df), T.pdf(vp, Yt, False, logflag, False, df), PDF_TOL[fam],
                 "%s pdf trans %s log=%d" % (tag, fam, logflag), plain=not logflag)
    for logflag in (True, False):
        y, dy = V.vbmc_pdf(vp, Y, False, logflag, nargout=2)
        ry, rdy = T.pdf(vp, Y, False, logflag, grad=True)
        same(y, ry, PDF_TOL["gauss"], "%s grad-call value log=%d" % (tag, logflag), plain=not logflag)
        err = float(np.max(np.abs(dy - rdy) / np.max(np.abs(rdy), axis=1, keepdims=True)))
        print("VPT-MEASURE edges %s gradient log=%d %.3e" % (tag, logflag, err))
        assert err <= GRAD_TOL, (tag, err)
    check_moments(V, vp, N, tag)
    check_kldiv(V, vp, T.sibling(vp, 2), N, tag)


# ---------------------------------------------------------------------------------------------------------------- a bad row stays in its lane
def test_a_bad_row_leaves_its_neighbours_alone(V):
    vp = T.make_case("G")
    N = 300                                                  # two full workgroups and a partial one; five waves
    B, _ = V.vp_rnd_rng_dump(SEED, N, vp["D"], vp["w"], True)
    X, _, Y = T.rnd(vp, N, True, True, B, SEED)
    tr = vp["trinfo"]
    lb, ub = np.asarray(tr["lb_orig"]), np.asarray(tr["ub_orig"])
    edits = [(0, lb[0] - 0.5), (0, ub[0] + 0.5), (2, lb[2] - 1.0), (3, ub[3] + 1.0), (4, np.nextafter(ub[4], np.inf)),   # outside
             (0, lb[0]), (0, ub[0]), (2, lb[2]), (3, ub[3]), (4, lb[4]),                                                 # on
             (1, 1e200), (1, -1e200), (1, 1e160)]                                                                        # huge
    bad = np.arange(0, N, 7)
    Xb = X.copy()
    for n, r in enumerate(bad):
        d, v = edits[n % len(edits)]
        Xb[r, d] = v
    Yb = Y.copy()
    Yb[bad] = T.warp(Xb[bad], "d", tr)                       # NaN, +-Inf and 1e200-sized rows of the transformed space
    keep = np.ones(N, dtype=bool)
    keep[bad] = False
    for fam, df in FAMILIES:
        for logflag in (True, False):
            clean, mixed = V.vbmc_pdf(vp, X, True, logflag, False, df), V.vbmc_pdf(vp, Xb, True, logflag, False, df)
            assert np.array_equal(clean[keep], mixed[keep]) and np.all(np.isfinite(clean)), (fam, logflag)
            nan = np.array([n % len(edits) < 10 for n in range(len(bad))])      # outside or on a bound: NaN; huge: -Inf resp. 0
            assert np.all(np.isnan(mixed[bad[nan]])) and np.all(mixed[bad[~nan]] == (-np.inf if logflag else 0.0)), (fam, logflag, mixed[bad])
    for logflag in (True, False):
        (y0, g0), (y1, g1) = V.vbmc_pdf(vp, Y, False, logflag, nargout=2), V.vbmc_pdf(vp, Yb, False, logflag, nargout=2)
        assert np.array_equal(y0[keep], y1[keep]) and np.array_equal(g0[keep], g1[keep]), logflag
        assert np.all(np.isfinite(g0)) and not np.any(np.isposinf(y1)), logflag
    again = V.vbmc_pdf(vp, X, True, True)                    # the context answers an ordinary call afterwards, unchanged
    assert np.array_equal(again, V.vbmc_pdf(vp, X, True, True, False, np.inf)) and np.all(np.isfinite(again))
    same(again, T.pdf(vp, X, True, True), PDF_TOL["gauss"], "after the bad rows")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_too_many_components_are_refused(V):
    import vbmc_amd

    vp = T.make_case("B")
    X = T.warp(np.asarray(vp["mu"]).T, "i", vp["trinfo"])
    ok = V.vbmc_pdf(vp, X, True, True)
    big, big2 = T.make_vp(2, 513, None, False), T.make_vp(2, 513, None, False, seed=2)
    small = T.make_vp(2, 512, None, False)
    calls = [lambda: V.vbmc_pdf(big, np.zeros((3, 2))), lambda: V.vbmc_pdf(big, np.zeros((3, 2)), False, True, nargout=2),
             lambda: V.vbmc_rnd(big, 10), lambda: V.vbmc_rnd(big, 10, True, True), lambda: V.vbmc_moments(big, True, 100),
             lambda: V.vbmc_kldiv(big, big2, 100), lambda: V.vbmc_kldiv(small, big, 100), lambda: V.vbmc_kldiv(big, small, 100)]
    for i, f in enumerate(calls):
        with pytest.raises(vbmc_amd.VbmcUnsupported):
            f()
        assert np.array_equal(V.vbmc_pdf(vp, X, True, True), ok), i
    assert np.all(np.isfinite(V.vbmc_pdf(small, np.zeros((3, 2)), True, True)))      # K = 512 itself is served

"""CPU: the NumPy restatement tests/_vptools_ref.py, which the GPU tests of the variational-posterior tools compare against, is itself
held to 50-digit values (tests/golden/mp_vptools_case{0..5}.json, written by tools/gen_vptools_golden.py) at the golden families'
1e-12, to closed forms (SciPy's multivariate normal, a density that integrates to one over its bounds), and to the properties of the
balanced split.  The host mirror vbmc_amd.vptools.warpvars is held to the same fixtures.  The randomness of every GPU case keeps the
margin from the cumulative weights that makes the component choice a matter of exact comparison, not of rounding."""
import json
import os
import re

import numpy as np
import pytest

from tests import _vptools_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
SEED = 20240607      # tests/test_gpu_vptools.py
NFIX = 6             # mp_vptools_case0 .. 5


def load(i):
    with open(os.path.join(ROOT, "tests", "golden", "mp_vptools_case%d.json" % i)) as f:
        g = json.load(f)
    vp = dict(g["vp"], trinfo=g["trinfo"])
    vp["mu"] = np.array(vp["mu"])
    return g, vp


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("i", range(NFIX))
def test_restatement_against_the_fixtures(i):
    g, vp = load(i)
    X, Y, tr = np.array(g["X"]), np.array(g["Y"]), g["trinfo"]
    close(T.warp(X, "d", tr), g["direct"], "direct")
    close(T.warp(Y, "i", tr), g["inverse"], "inverse")
    close(T.warp(Y, "l", tr), g["logjac"], "logjac")
    close(T.warp(Y, "p", tr), np.exp(g["logjac"]), "jac")
    close(T.pdf(vp, X, True, True), g["logpdf_orig"], "log pdf, original space")
    assert np.max(np.abs(T.pdf(vp, X, True, False) / np.array(g["pdf_orig"]) - 1)) <= TOL
    close(T.pdf(vp, Y, False, True), g["logpdf_trans"], "log pdf, transformed space")
    close(T.pdf(vp, Y, True, True, True), np.array(g["logpdf_trans"]) - np.array(g["logjac"]), "log pdf, transflag")
    for df in g["dfs"]:
        close(T.pdf(vp, X, True, True, False, df), g["heavy"][str(df)], "t family df = %g" % df)
    if g["grad"] is not None:
        _, dy = T.pdf(vp, Y, False, False, grad=True)
        _, dl = T.pdf(vp, Y, False, True, grad=True)
        scale = np.max(np.abs(g["grad"]), axis=1, keepdims=True)
        assert np.max(np.abs(dy - np.array(g["grad"])) / scale) <= TOL
        close(dl, g["gradlog"], "gradient of the log density")


def test_fixtures_cover_what_they_should():
    types, rot, dfs, grads = set(), 0, [], 0
    for i in range(NFIX):
        g, _ = load(i)
        assert g["vp"]["D"] <= 7 and g["vp"]["K"] <= 4 and len(g["X"]) <= 8
        if g["trinfo"]:
            types |= set(g["trinfo"]["type"])
            rot += g["trinfo"]["R_mat"] is not None and g["trinfo"]["scale"] is not None
        dfs += g["dfs"]
        grads += g["grad"] is not None
    assert types == {0, 1, 2, 3} and rot >= 1 and any(d > 0 for d in dfs) and any(d < 0 for d in dfs) and grads >= 1


@pytest.mark.parametrize("i", range(NFIX))
def test_host_mirror_against_the_fixtures(i):
    from vbmc_amd.vptools import warpvars

    g, _ = load(i)
    X, Y, tr = np.array(g["X"]), np.array(g["Y"]), g["trinfo"]
    close(warpvars(X, "dir", tr), g["direct"], "direct")
    close(warpvars(Y, "inv", tr), g["inverse"], "inverse")
    close(warpvars(Y, "logprob", tr), g["logjac"], "logjac")
    close(warpvars(Y, "prob", tr), np.exp(g["logjac"]), "jac")


@pytest.mark.parametrize("name", list(T.CASES))
def test_inverse_of_direct_is_the_identity(name):
    vp = T.make_case(name)
    r = np.random.default_rng(3)
    Y = np.asarray(vp["mu"]).T[r.integers(0, vp["K"], 50)] + 0.3 * r.normal(size=(50, vp["D"]))
    X = T.warp(Y, "i", vp["trinfo"])
    assert np.max(np.abs(T.warp(X, "d", vp["trinfo"]) - Y)) <= 1e-9 * max(1.0, np.max(np.abs(Y)))   # (the logit amplifies a rounding of x)
    assert np.max(np.abs(T.warp(T.warp(X, "d", vp["trinfo"]), "i", vp["trinfo"]) - X) / np.maximum(1.0, np.abs(X))) <= 1e-13


def test_single_gaussian_against_scipy():
    from scipy.stats import multivariate_normal

    r = np.random.default_rng(0)
    D = 3
    vp = dict(D=D, K=1, mu=r.normal(size=(D, 1)), sigma=np.array([0.7]), w=np.array([1.0]), trinfo=None)
    vp["lambda"] = np.array([0.5, 1.0, 1.7])
    X = r.normal(size=(20, D))
    ref = multivariate_normal(mean=vp["mu"][:, 0], cov=np.diag((0.7 * vp["lambda"]) ** 2))
    assert np.allclose(T.pdf(vp, X, True, True), ref.logpdf(X), rtol=0, atol=1e-12)
    assert np.allclose(T.pdf(vp, X, False, False), ref.pdf(X), rtol=1e-12, atol=0)


def test_logit_posterior_integrates_to_one():
    from scipy.integrate import quad

    vp = dict(D=1, K=2, mu=np.array([[-0.5, 0.8]]), sigma=np.array([0.6, 0.4]), w=np.array([0.3, 0.7]),
              trinfo=dict(lb_orig=[-1.0], ub_orig=[3.0], type=[3], mu=[0.2], delta=[1.3], scale=None, R_mat=None))
    vp["lambda"] = np.array([1.0])
    val, err = quad(lambda x: float(T.pdf(vp, [[x]], True, False)[0]), -1.0, 3.0, epsabs=1e-11, epsrel=1e-11, limit=200)
    assert abs(val - 1.0) <= 1e-9, (val, err)


@pytest.mark.parametrize("N", T.POINT_COUNTS + (70000,))
def test_balanced_split(N):
    r = np.random.default_rng(N)
    w = np.ravel(T.make_case("D")["w"])
    K = w.size
    u = r.random(N + K)
    I_all, M0 = T.split(w, N, True, u)
    n_floor = np.floor(w * N).astype(int)
    assert M0 == n_floor.sum() and N <= I_all.size <= N + K
    assert np.array_equal(np.bincount(I_all[:M0], minlength=K), n_floor)                  # exactly floor(w N) of each ...
    assert np.array_equal(np.bincount(I_all, minlength=K), n_floor + np.bincount(I_all[M0:], minlength=K))   # ... plus the remainder's
    pi = T.perm(SEED, I_all.size, N)
    assert len(set(pi.tolist())) == N and pi.min() >= 0 and pi.max() < I_all.size         # a bijection onto N of the M samples
    if I_all.size == N:
        assert np.array_equal(np.sort(pi), np.arange(N))
    assert not np.array_equal(pi, np.arange(N)) or N == 1


def test_catrnd_margins_of_the_gpu_cases():
    """Every catrnd decision of every GPU case stays 1e-9 (relative) away from each cumulative weight: the device's choice of a
    component cannot hinge on the rounding of a product."""
    from vbmc_amd.vptools import vp_rnd_rng_dump

    smallest = np.inf
    runs = [(name, 1003, bal, SEED) for name in T.CASES for bal in (False, True)] + [(name, 65, True, SEED) for name in T.CASES]
    runs += [("B", N, True, SEED) for N in (1, 63, 64, 65, 70000)] + [("C", N, False, SEED) for N in (1, 63, 64, 65, 70000)]
    runs += [("D", 70000, True, SEED), ("D", 70000, True, SEED + 1), ("D", 65536, True, SEED), ("B", 2, True, SEED)]
    runs += [(name, 1003, True, SEED + 1) for name in T.CASES]                            # kldiv's second direction
    for name, N, bal, seed in runs:
        vp = T.make_case(name)
        for v in (vp, T.sibling(vp, 2), T.sibling(vp, 3, T.NARROW["width"], same_mu=True)):
            B, _ = vp_rnd_rng_dump(seed, N, v["D"], v["w"], bal)
            smallest = min(smallest, T.catrnd_margin(v["w"], N, bal, B[:, 0]))
    print("smallest margin %.3e" % smallest)
    assert smallest >= 1e-9, smallest


def test_cases_reach_every_width_and_a_chunk_seam():
    """The GPU cases launch all six padded widths of vpt_pick_dt and, at every width from 8 on, a mixture with more components than
    one staged chunk of 2048 / DT holds (at 4 the chunk is the largest K there is)"""
    shapes = [(T.padded_width(D), K) for D, K, _, _ in T.CASES.values()]
    assert {dt for dt, _ in shapes} == set(T.PADDED_WIDTHS), shapes
    for dt in T.PADDED_WIDTHS:
        assert dt == 4 or any(d == dt and K > T.CHUNK_DOUBLES // dt for d, K in shapes), (dt, shapes)
    assert any(d == dt and K == T.CHUNK_DOUBLES // dt + 1 for d, K in shapes for dt in (8, 12, 16))      # a last chunk of one component
    assert any(K > 2 * (T.CHUNK_DOUBLES // d) for d, K in shapes)                                          # three chunks or more
    with open(os.path.join(ROOT, "vbmc_amd", "csrc", "vp_tools_host.h")) as f:                         # the mirrored constants
        m = re.search(r"\bdts\s*\[\s*\]\s*=\s*\{([^}]*)\}", f.read())
        assert m and tuple(int(v) for v in m.group(1).split(",")) == T.PADDED_WIDTHS
    with open(os.path.join(ROOT, "vbmc_amd", "csrc", "vp_tools_kernels.h")) as f:
        m = re.search(r"#\s*define\s+VPT_CHUNK\s+(\d+)", f.read())
        assert m and int(m.group(1)) == T.CHUNK_DOUBLES


def test_band_fixture_keeps_clear_of_the_threshold():
    """tests/golden/mp_vptools_band.json: the log of the transformed-space mixture reaches its targets on both sides of log(realmin) and
    of log(5e-324), and no stored value lies within 1e-6 of the latter; the restatement agrees where its sum is a normal number"""
    with open(os.path.join(ROOT, "tests", "golden", "mp_vptools_band.json")) as f:
        g = json.load(f)
    thr = g["threshold"]
    assert thr == -744.4400719213812 and abs(np.exp(thr) / 5e-324 - 1) < 1 and len(g["mixtures"]) == 2
    targets = [-690, -705, -708.3, -708.5, -720, -740, -744.3, -744.6, -745.2, -760, -1000, -1e5]
    for m in g["mixtures"]:
        lm, lo = np.array(m["logmix_trans"]), np.array(m["logpdf_orig"])
        assert np.max(np.abs(lm[:len(targets)] - targets)) <= 0.05 and len(m["X"]) == len(targets) + 2
        assert np.min(np.abs(lm - thr)) > 1e-6 and np.min(np.abs(lo - thr)) > 1e-6
        assert np.sum(lm > thr) >= 9 and np.sum(lm < thr) >= 5 and np.all(np.isfinite(lo))
        vp = dict(m["vp"], trinfo=m["trinfo"])
        vp["mu"] = np.array(vp["mu"])
        normal = lm > -708.0
        close(T.pdf(vp, np.array(m["X"]), True, True)[normal], lo[normal], "band, log pdf")
        for df in g["dfs"]:
            assert np.all(np.isfinite(m["heavy"][str(df)]))
            close(T.pdf(vp, np.array(m["X"]), True, True, False, df), m["heavy"][str(df)], "band, t family df = %g" % df)


def test_edge_rows_are_what_they_claim():
    """The inputs of tests/test_gpu_vptools_edges.py on the restatement alone: subnormal distances from a bound, logit arguments next to 0
    and 1, NaN on and beyond a bound; a caller block of +-1e3 normals reaches both clamp ends exactly and +Inf"""
    from vbmc_amd.vptools import vp_rnd_rng_dump

    vp = T.make_zero_bounds()
    near, huge, on, out = T.zero_bounds_rows()
    y = T.warp(near, "d", vp["trinfo"])
    assert np.all(near[1:3, 0] < 2.3e-308) and np.all(near[1:3, 0] > 0) and np.all(-near[3:5, 1] < 2.3e-308) and np.all(near[3:5, 1] < 0)
    assert np.allclose([y[1, 0], y[2, 0], y[3, 1], y[4, 1]], np.log(2.0) * np.array([-1060, -1030, -1060, -1030]), rtol=1e-15)
    assert np.all(np.isfinite(T.pdf(vp, near, True, True)))                        # (a wide component sits there)
    vl = T.make_logit()
    lnear, lhuge, lon, lout = T.logit_rows()
    tr = vl["trinfo"]
    z = (lnear[1:, 0] - tr["lb_orig"][0]) / (tr["ub_orig"][0] - tr["lb_orig"][0])
    assert np.array_equal(z, [2.0 ** -40, 2.0 ** -52, 1 - 2.0 ** -40, 1 - 2.0 ** -52])
    assert np.all(np.isfinite(T.pdf(vl, lnear, True, True)))
    for v, hg, o, ou in ((vp, huge, on, out), (vl, lhuge, lon, lout)):
        for logflag in (True, False):
            r = T.pdf(v, hg, True, logflag)
            assert np.isfinite(r[0]) and np.all(r[1:] == (-np.inf if logflag else 0.0))
            for rows in (o, ou):
                r = T.pdf(v, rows, True, logflag)
                assert np.isfinite(r[0]) and np.all(np.isnan(r[1:])), (rows, r)
    Yt = T.logit_trans_rows(vl, [s * z for z in T.LOGIT_Z for s in (1.0, -1.0) if s * z > -T.LOGIT_Z_REF_OVERFLOWS])
    zz = Yt[1:, 0] * tr["delta"][0] + tr["mu"][0]
    assert np.sum(1.0 + np.exp(-np.abs(zz)) == 1.0) >= 8 and np.sum(np.exp(-np.abs(zz)) == 0.0) >= 2 and np.sum(np.abs(zz) > 745) >= 2
    r = T.pdf(vl, Yt, True, True, True)
    assert not np.any(np.isnan(r)) and np.sum(np.isfinite(r)) >= 9                 # (the wide components again)
    # the clamp
    vc = T.make_clamp()
    lo, hi = T.clamp_ends(vc["trinfo"])
    for bal in (False, True):
        B, perm = vp_rnd_rng_dump(SEED, 65, 4, vc["w"], bal)
        X = T.rnd(vc, 65, True, bal, T.clamp_block(B, perm), SEED)[0]
        up, down = [r for r, v in T.CLAMP_ROWS if v > 0], [r for r, v in T.CLAMP_ROWS if v < 0]
        assert np.all(X[up, 1] == np.inf) and np.all(X[up, 2] == -np.inf) and np.all(X[up, 3] == hi[3])
        assert np.all(X[down, 1] == lo[1]) and np.all(X[down, 2] == hi[2]) and np.all(X[down, 3] == lo[3])
        assert np.all(np.isfinite(X[:, 0])) and np.all(X >= lo) and np.all(X <= hi)
        assert T.catrnd_margin(vc["w"], 65, bal, B[:, 0]) >= 1e-9
    # zero weights: the margin of the component choice
    for which in T.ZERO_WEIGHTS:
        vz = T.make_zero_weight(which)
        assert np.all(vz["w"][list(which)] == 0) and abs(vz["w"].sum() - 1) < 1e-15
        for v, seed in ((vz, SEED), (vz, SEED + 1), (T.sibling(vz, 2), SEED + 1)):
            for bal in (False, True):
                B, _ = vp_rnd_rng_dump(seed, 1003, 5, v["w"], bal)
                assert T.catrnd_margin(v["w"], 1003, bal, B[:, 0]) >= 1e-9
                assert not np.isin(T.split(v["w"], 1003, bal, B[:, 0])[0], [k for k in range(4) if v["w"][k] == 0]).any()


def test_narrow_case_exercises_the_floor_rule():
    """vbmc_kldiv.m:76 acts on 1-20 % of vp1's draws in the narrow case of tests/test_gpu_vptools.py"""
    from vbmc_amd.vptools import vp_rnd_rng_dump

    vp1 = T.make_case(T.NARROW["case"])
    vp2 = T.sibling(vp1, 3, T.NARROW["width"], same_mu=True)
    B1, _ = vp_rnd_rng_dump(SEED, 1003, vp1["D"], vp1["w"], True)
    B2, _ = vp_rnd_rng_dump(SEED + 1, 1003, vp2["D"], vp2["w"], True)
    x1, x2 = T.rnd(vp1, 1003, True, True, B1, SEED)[0], T.rnd(vp2, 1003, True, True, B2, SEED + 1)[0]
    kls, share = T.kldiv_terms(vp1, vp2, x1, x2)
    assert 0.01 <= share[0] <= 0.20, share
    assert np.all(np.isfinite(kls)) and np.all(kls >= 0)


def test_mvnkl_and_moments():
    r = np.random.default_rng(1)
    A, B = r.normal(size=(3, 3)), r.normal(size=(3, 3))
    S1, S2, m1, m2 = A @ A.T + np.eye(3), B @ B.T + np.eye(3), r.normal(size=3), r.normal(size=3)
    k1, k2 = T.mvnkl(m1, S1, m2, S2)
    assert k1 > 0 and k2 > 0 and np.allclose(T.mvnkl(m1, S1, m1, S1), 0.0, atol=1e-12)
    from vbmc_amd.vptools import mvnkl

    assert np.allclose(mvnkl(m1, S1, m2, S2), (k1, k2), rtol=1e-13)
    # the shifted sums the device forms against cov
    X = r.normal(size=(1003, 3)) * [1.0, 5.0, 0.1] + [100.0, -3.0, 0.5]
    c = X[0] + 0.1
    Xc = X - c
    s1, s2 = Xc.sum(0), Xc.T @ Xc
    cov = (s2 - np.outer(s1, s1) / len(X)) / (len(X) - 1)
    mu, S = T.moments(X)
    sd = np.sqrt(np.diag(S))
    assert np.max(np.abs(cov - S) / np.outer(sd, sd)) <= 1e-12 and np.max(np.abs(c + s1 / len(X) - mu) / sd) <= 1e-12

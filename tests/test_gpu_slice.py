"""GPU: the device-resident slice sampler (vbmc_gp_slice_sample) against the NumPy restatement of slicesamplebnd
(tests/_slice_ref.py) fed the oracle's gplite_nlZ with hprior as target and the same indexed uniform block (parity mode).

Given identical accept / reject decisions a sample is an affine function of the uniforms, so samples and widths are held to the
project's value tolerance 1e-10 (relative, scaled as tests/test_gpu_nlz.py scales it) and logp to that file's tolerance for nlZ
against the oracle -- `abs(nlZ - f) < 1e-10 * max(1.0, abs(f))`, tests/test_gpu_nlz.py:73,93: the same 1e-10, NLZ_TOL below; a flipped decision would show as an error of the order of a width.  Seeds are fixed per case (no case is
skipped for a near-tie; none of these seeds produces one)."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._slice_ref import SliceCollapse, make_block, slicesamplebnd
from tests.test_gpu_nlz import make_gp

pytestmark = pytest.mark.gpu

KMAX = 40
NLZ_TOL = 1e-10      # tests/test_gpu_nlz.py:73,93 (nlZ against the oracle)


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


# N, D, meanfun, noisefun, s2 present, Ns, Thin, Burnin, Adaptive, fixed coordinate, coordinate started next to its bound, seed
CASES = [
    (40, 2, 0, (1, 0, 0), False, 8, 1, 10, True, None, None, 101),
    (60, 3, 1, (1, 1, 0), True, 3, 5, 0, False, 1, None, 102),
    (50, 2, 4, (1, 2, 0), True, 6, 1, 8, True, 0, 3, 103),
    (45, 3, 4, (1, 0, 1), False, 4, 5, 6, True, None, 2, 104),
    (33, 2, 4, (1, 2, 1), True, 5, 1, 7, False, 4, 0, 105),
    (80, 4, 1, (0, 1, 0), True, 4, 1, 5, True, None, None, 106),
    # the sizes at which the kernels take a second trip through their strided loops or the factorisation another form
    (70, 21, 4, (1, 0, 0), False, 2, 1, 4, True, None, None, 107),    # Nhyp = 66
    (70, 21, 4, (1, 0, 0), False, 2, 1, 4, True, 64, 65, 108),        # ... coordinate 64 fixed, coordinate 65 started next to its bound
    (300, 3, 1, (1, 1, 0), True, 2, 1, 2, True, None, None, 109),     # 256 < N <= 512, s2 different per point
    (565, 3, 1, (1, 0, 1), False, 2, 1, 2, True, None, None, 110),    # N > 512 and > 560 (the N of tests/_trainopt_cases.py)
]
WIDE = [6, 7, 8, 9]


def problem(case):
    N, D, meanfun, nf, has_s2, Ns, thin, burn, adaptive, fixed, near, seed = case
    rng = np.random.default_rng(seed)
    gp, draw = make_gp(rng, N, D, meanfun, (nf[0] or 1, nf[1], nf[2]))
    if nf[0] == 0:      # no constant-noise hyper-parameter: drop it from the vector make_gp draws
        gp["noisefun"] = tuple(nf)
        gp["Nnoise"] = R.noisefun_nhyp(nf)
        h = np.delete(draw(), D + 1)
        gp["s2"] = gp["s2"] + 0.02
    else:
        h = draw()
    if not has_s2:
        gp["s2"] = None
    Nhyp = h.size
    assert Nhyp == gp["Ncov"] + gp["Nnoise"] + gp["Nmean"]
    LB = h - 2.5
    UB = h + 2.5
    LB[0], UB[Nhyp - 1] = -np.inf, np.inf
    x0 = h.copy()
    if fixed is not None:
        LB[fixed] = UB[fixed] = h[fixed]
    if near is not None:
        x0[near] = np.nextafter(LB[near], np.inf) if np.isfinite(LB[near]) else h[near]
        if near == 0:
            LB[0] = h[0] - 1.0
            x0[0] = LB[0] + 1e-12
    hp = {"mu": h + 0.3, "sigma": 2.0 * np.ones(Nhyp), "df": np.array(([3.0, 0.0, np.inf, 7.0] * Nhyp)[:Nhyp])}
    hp["mu"][Nhyp - 1] = np.nan          # a flat prior on the last coordinate
    widths = 0.4 + 0.2 * rng.random(Nhyp)
    sweeps = burn + Ns + (Ns - 1) * (thin - 1)
    perms, U = make_block(rng, sweeps, Nhyp, KMAX)
    opts = {"Thin": thin, "Burnin": burn, "Adaptive": adaptive}
    return gp, hp, x0, Ns, widths, LB, UB, opts, perms, U


def oracle_chain(gp, hp, x0, Ns, widths, LB, UB, opts, perms, U):
    def logf(x):          # gp_objfun with swapsign (gplite_train.m:318,516-546): anything that goes wrong is a NaN
        try:
            return -float(R.gplite_nlZ(x, gp, hp, compute_grad=False)[0])
        except (np.linalg.LinAlgError, ValueError, FloatingPointError):
            return np.nan

    return slicesamplebnd(logf, x0, Ns, widths, LB, UB, opts, perms, U)


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _case_id(c):
    return "N%d_D%d_m%d_nf%d%d%d_thin%d_burn%d" % (c[0], c[1], c[2], *c[3], c[6], c[7]) + ("_fixed%d" % c[9] if (c[9] or 0) >= 64 else "")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_parity_with_the_restatement(va, case):
    """The first six cases are D <= 4, N <= 80, Nhyp <= 15.  The last four take the seams of the kernels behind the chain:
    Nhyp = 66 > 64 (the second trip of k_slice_decide's lanes over the coordinates: sample recording, xsum / xsq, the q = 1 slot of
    the end-of-burn-in width adaptation, and -- every case here passes widths, so has_base is set -- its base-width branch; the
    hyper-prior of gpobj_emit beyond lane 63), one of them with coordinate 64 fixed and coordinate 65 started next to its bound;
    256 < N <= 512 (N = 300 with s2: gpobj_emit's noise loop beyond its 256 threads); N = 565 > 560 (k_alpha_solve, two Cholesky
    panels, output-dependent noise).  Ninit and syrk_form belong to the optimiser alone (tests/test_gpu_trainopt.py).
    Oracle evaluations on the CPU: 487, 461, 40, 49; no accept decision of these seeds changes under a 1e-9 relative perturbation
    of the target, so none was passed over.  Seen on an MI355X when they went in: samples and widths equal to the last bit, logp
    within 8.9e-16, 1.4e-15, 2.6e-15 and 2.0e-13."""
    gp, hp, x0, Ns, widths, LB, UB, opts, perms, U = problem(case)
    rs, rf, ro = oracle_chain(gp, hp, x0, Ns, widths, LB, UB, opts, perms, U)
    s, f, flag, out = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=4)
    es = np.max(np.abs(s - rs) / np.maximum(1.0, np.abs(rs)))
    ef = np.max(np.abs(f - rf) / np.maximum(1.0, np.abs(rf)))
    ew = np.max(np.abs(out.widths - ro["widths"]) / np.maximum(1.0, np.abs(ro["widths"])))
    print("slice parity: samples %.2e logp %.2e widths %.2e funccount %d/%d maxshrink %d/%d performed %d"
          % (es, ef, ew, out.funccount, ro["funccount"], out.maxshrink, ro["maxshrink"], out.performed))
    assert flag == 0
    assert close(s, rs, 1e-10), es
    assert close(out.widths, ro["widths"], 1e-10), ew
    assert close(f, rf, NLZ_TOL), ef
    assert out.funccount == ro["funccount"] and out.maxshrink == ro["maxshrink"]
    fixed = LB == UB
    assert np.all(s[:, fixed] == x0[fixed]) and np.all(s >= LB) and np.all(s <= UB)
    if not opts["Adaptive"]:
        assert np.array_equal(out.widths[~fixed], widths[~fixed])


@pytest.mark.parametrize("ci,Ws", [pytest.param(0, (1, 2, 8, 16), id="0"), pytest.param(2, (1, 2, 8, 16), id="2"), pytest.param(4, (1, 2, 8, 16), id="4"),
                                   pytest.param(6, (1, 16), id="6")])     # (6: Nhyp = 66)
def test_speculation_width_does_not_change_a_bit(va, ci, Ws):
    gp, hp, x0, Ns, widths, LB, UB, opts, perms, U = problem(CASES[ci])
    ref = None
    performed = []
    for W in Ws:
        s, f, _, out = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=W)
        performed.append(out.performed)
        if ref is None:
            ref = (s, f, out)
            assert out.performed == out.funccount           # W = 1 launches exactly what the sequential chain needs
            continue
        assert np.array_equal(s, ref[0]) and np.array_equal(f, ref[1]) and np.array_equal(out.widths, ref[2].widths), W
        assert out.funccount == ref[2].funccount and out.maxshrink == ref[2].maxshrink
    assert performed[-1] > performed[0]


def test_device_rng_replays_through_its_dump(va):
    gp, hp, x0, Ns, widths, LB, UB, opts, _, _ = problem(CASES[2])
    sweeps = opts["Burnin"] + Ns + (Ns - 1) * (opts["Thin"] - 1)
    s1, f1, _, o1 = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, seed=77, W=2)
    perms, U = va.slice_rng_dump(77, sweeps, x0.size, max(o1.maxshrink, 1))
    s2, f2, _, o2 = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=2)
    assert np.array_equal(s1, s2) and np.array_equal(f1, f2) and np.array_equal(o1.widths, o2.widths)
    assert (o1.funccount, o1.maxshrink) == (o2.funccount, o2.maxshrink)
    s3, _, _, _ = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, seed=78, W=2)
    assert not np.array_equal(s1, s3)
    # ... and the device-mode chain is the restatement's chain on that block
    rs, rf, ro = oracle_chain(gp, hp, x0, Ns, widths, LB, UB, opts, perms, U)
    assert close(s1, rs, 1e-10) and close(f1, rf, 1e-10) and o1.funccount == ro["funccount"]


def test_errors_leave_the_context_usable(va):
    gp, hp, x0, Ns, widths, LB, UB, opts, perms, U = problem(CASES[0])

    def still_works():
        v = va.gplite_nlZ(x0, gp, hp, nargout=1)
        r = R.gplite_nlZ(x0, gp, hp, compute_grad=False)[0]
        assert abs(v - r) < 1e-10 * max(1.0, abs(r))

    # the interval collapses onto the current point: slice level AT log_Px (rand = 1), interval starting AT the point (rand = 0),
    # proposal AT the interval's start (rand = 0) -- the reference's error (:298-301), in the restatement and on the device
    Uc = U.copy()
    Uc[0, 0, :] = 0.0
    Uc[0, 0, 0] = 1.0
    with pytest.raises(SliceCollapse):
        oracle_chain(gp, hp, x0, Ns, widths, LB, UB, opts, perms, Uc)
    with pytest.raises(va.VbmcHipError, match="Shrunk to current position and proposal still not acceptable") as e:
        va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=Uc, perms=perms, W=4)
    assert e.value.status == va._lib.VBMC_ERR_INVALID
    still_works()
    # an out-of-range argument
    bad = x0.copy()
    bad[1] = UB[1] + 1.0
    with pytest.raises(va.VbmcHipError, match="outside the bounds") as e:
        va.slicesamplebnd_gp(gp, hp, bad, Ns, widths, LB, UB, opts, uniforms=U, perms=perms)
    assert e.value.status == va._lib.VBMC_ERR_INVALID
    with pytest.raises(va.VbmcHipError) as e:
        va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=17)
    assert e.value.status == va._lib.VBMC_ERR_INVALID
    still_works()
    # an unsupported mean function
    with pytest.raises(va.VbmcUnsupported):
        va.slicesamplebnd_gp(dict(gp, meanfun=6), hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms)
    still_works()
    # a uniform block too short for the chain is an error, not a hang
    with pytest.raises(va.VbmcHipError, match="uniform block exhausted"):
        va.slicesamplebnd_gp(gp, hp, x0, Ns, 50.0 * np.ones(x0.size), LB, UB, dict(opts, Adaptive=False), uniforms=U[:, :, :3], perms=perms)
    still_works()


def test_gplite_train_sample_end_to_end(va):
    from tests.test_gpu_elbo import relerr

    gp, hp, x0, _, widths, LB, UB, _, _, _ = problem(CASES[3])
    Ns, Thin = 4, 3
    new, hyp, out = va.gplite_train_sample(gp, x0, Ns, hp, LB, UB, widths, Thin=Thin, Burnin=6, seed=5, need_L=False)
    assert hyp.shape == (x0.size, Ns) and out["hyp_prethin"].shape == (x0.size, Ns * Thin)
    assert np.array_equal(hyp, out["hyp_prethin"][:, Thin - 1::Thin]) and np.array_equal(out["logp"], out["logp_prethin"][Thin - 1::Thin])
    assert len(new["post"]) == Ns and all(p["L"] is None for p in new["post"])          # need_L=False: no L crosses to the host
    assert all(np.array_equal(p["hyp"], hyp[:, s]) for s, p in enumerate(new["post"]))
    rng = np.random.default_rng(0)
    Xs = 1.2 * rng.standard_normal((25, gp["X"].shape[1]))
    ref = va.gplite_post(hyp, gp["X"], gp["y"], 1, gp["meanfun"], gp["noisefun"], gp["s2"])
    a = va.gplite_pred(new, Xs, None, None, True)
    b = va.gplite_pred(ref, Xs, None, None, True)
    for x, z in zip(a, b):
        assert relerr(x, z) < 1e-7
    o = R.gplite_pred(R.gplite_post(hyp, gp["X"], gp["y"], meanfun=gp["meanfun"], noisefun=gp["noisefun"], s2=gp["s2"]), Xs, ssflag=True)
    assert relerr(a[2], o[2]) < 1e-7 and relerr(a[3], o[3]) < 1e-6
    # the recorded log posterior is the target at the recorded point
    for s in range(Ns):
        r = -R.gplite_nlZ(hyp[:, s], gp, hp, compute_grad=False)[0]
        assert abs(out["logp"][s] - r) < 1e-10 * max(1.0, abs(r))


def test_failed_factorisations_inside_the_chain(va):
    """The stall / checked-round path: twenty exactly duplicated training points make K singular, and in every sweep the noise
    coordinate's first proposal is steered (parity uniforms: placement 0.9, first shrink rand 0.05, width 200) about 170 below the
    current log noise, where sn2 ~ 1e-150 is lost against the diagonal even after the nine x10 inflations: the factorisation fails
    all ten tries in the oracle and on the device, the target is NaN (gplite_train.m:542-546), a rejected proposal that COUNTS
    (slicesamplebnd.m:440-443).  The coordinate's later rands lie in [0.99, 1): those proposals fall within 1.72 of the interval's
    upper end, where (asserted below, on the oracle's side) sn2 >= 1e-6: the branch whose matrix K/sn2 + I cannot fail, so every value
    that decides anything is well conditioned and the usual tolerances hold.  Nothing is compared where only coarse agreement is meaningful (a matrix that passes
    after some inflations, tests/test_gpu_nlz.py:107-119): no proposal lands there."""
    N, D = 50, 3
    rng = np.random.default_rng(314)
    gp, draw = make_gp(rng, N, D, 4, (1, 0, 0))
    gp["X"] = np.vstack([gp["X"][:30], gp["X"][:20]])
    gp["y"] = np.concatenate([gp["y"][:30], gp["y"][:20]])
    h = draw()
    Nhyp, inoise = h.size, D + 1
    LB, UB = h - 2.5, h + 2.5
    LB[inoise], UB[inoise] = h[inoise] - 400.0, h[inoise] + 1.0
    hp = {"mu": h + 0.3, "sigma": 2.0 * np.ones(Nhyp), "df": np.array(([3.0, 0.0, np.inf, 7.0] * Nhyp)[:Nhyp])}
    hp["mu"][inoise], hp["sigma"][inoise], hp["df"][inoise] = h[inoise], 0.3, 0.0      # (keeps the chain from drifting to low noise)
    widths = 0.4 + 0.2 * rng.random(Nhyp)
    widths[inoise] = 200.0
    Ns, opts = 5, {"Thin": 1, "Burnin": 0, "Adaptive": False}
    perms, U = make_block(rng, Ns, Nhyp, KMAX)
    for sw in range(Ns):
        idd = int(np.nonzero(perms[sw] == inoise)[0][0])
        U[sw, idd, 1] = 0.9
        U[sw, idd, 2] = 0.05
        U[sw, idd, 3:] = 0.99 + 0.01 * rng.random(KMAX - 1)
    nan_calls = {"n": 0}

    def logf(x):
        v = -float(R.gplite_nlZ(x, gp, hp, compute_grad=False)[0])
        nan_calls["n"] += int(np.isnan(v))
        if not np.isnan(v):
            nan_calls["low"] = min(nan_calls.get("low", np.inf), x[inoise])
        return v

    rs, rf, ro = slicesamplebnd(logf, h, Ns, widths, LB, UB, opts, perms, U)
    assert nan_calls["n"] == Ns                                    # one hopeless proposal per sweep, NaN in the oracle
    assert nan_calls["low"] > 0.5 * np.log(1e-6)                 # every other proposal on the Cholesky branch (sn2 >= 1e-6)
    outs = {}
    for W in (1, 8):
        s, f, _, out = va.slicesamplebnd_gp(gp, hp, h, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=W)
        outs[W] = (s, f, out)
        print("slice stall W=%d: funccount %d/%d performed %d maxshrink %d/%d" % (W, out.funccount, ro["funccount"], out.performed,
                                                                              out.maxshrink, ro["maxshrink"]))
        assert close(s, rs, 1e-10) and close(f, rf, 1e-10)
        assert out.funccount == ro["funccount"] and out.maxshrink == ro["maxshrink"]
    # W = 1: every hopeless candidate was launched twice, optimistically and in the checked round with the retries
    assert outs[1][2].performed == outs[1][2].funccount + Ns
    assert np.array_equal(outs[1][0], outs[8][0]) and np.array_equal(outs[1][1], outs[8][1])

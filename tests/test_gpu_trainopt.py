"""vbmc_gp_train_optimize (the optimisation half of gplite_train on the device) against its NumPy restatement
(tests/_trainopt_ref.py) driven by the device's own gplite_nlZ through the ABI, its invariance under the speculation width, the
first-order condition at what it returns, the failed-factorisation paths and the reference's own known answers
(test/runtest_vbmc.m) with gplite_train in the place of the scipy stand-in of tests/test_gpu_known_answers.py."""
import functools

import numpy as np
import pytest

from tests import _trainopt_ref as T
from tests._trainopt_cases import PARITY_CASES, PARITY_NINIT, PARITY_NOPTS, WIDE_CASES, gp_case, parity_case, parity_sizes

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-9      # the project's gradient-level tolerance
TOL_FILL = 1e-10


def _device_fun(va, c):
    def fun(h):
        f, g = va.gplite_nlZ(np.asarray(h, dtype=np.float64), c["gp"], c["hprior"], 2)
        f = float(f)
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        return (f, g) if np.isfinite(f) else (np.nan, np.full(g.size, np.nan))
    return fun


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def _optimized(ci):
    """(case, design, the device's result) of parity case ci with W = 2: one device run for the tests that read it (none writes to it)"""
    import vbmc_amd as va

    c, tol, maxit = parity_case(ci)
    Ninit, Nopts = parity_sizes(ci)
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], Ninit, seed=3)
    out = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"],
                                   {"Design": design, "Nopts": Nopts, "TolFun": tol, "MaxIter": maxit, "W": 2, "History": 128})
    return c, design, out


@pytest.mark.parametrize("ci", range(len(PARITY_CASES)))
def test_parity_with_the_restatement(ci):
    """The cases were chosen on the CPU with the oracle's gplite_nlZ as the objective (tests/_trainopt_cases.py states the two
    conditions, tests/test_trainopt_restatement.py asserts them): no Armijo or stopping decision of the restatement within 1e-6
    relative of flipping, no two fill values closer than 1e-6, and a trajectory that a 1e-13 perturbation of the gradient moves by
    less than 1e-10.  The first condition is asserted here too, on the run driven by the device objective.

    Cases 0-7 are D <= 2, N <= 40, Nhyp <= 11, Ninit = 24, Nopts = 2.  Cases 8 on (tests/_trainopt_cases.py says what each is for)
    cover the sizes at which the kernels take another trip or another form: Nhyp = 66 > 64 (8, 9, 10), a fixed coordinate at index
    64 (10), 256 < N <= 512 (11: N = 300 with s2), N > 560 (12, 13: N = 565), syrk_form 2 with sixteen starts (14), Ninit = 300 with a
    ragged second fill chunk (15) and Ninit = 1024 (16)."""
    import vbmc_amd as va

    _, tol, maxit = parity_case(ci)
    Ninit, Nopts = parity_sizes(ci)
    c, design, out = _optimized(ci)
    margin = []
    ref = T.train_optimize(_device_fun(va, c), design, Nopts, c["gp"]["Ncov"], c["gp"]["Nnoise"], c["LB"], c["UB"], tol, MaxIter=maxit, margin=margin)
    fin = ref["fill_fvals"][np.isfinite(ref["fill_fvals"])]
    assert min(margin) > 1e-6 and np.min(np.diff(fin)) > 1e-6, (min(margin), np.min(np.diff(fin)))
    print("case %d: fill err %.2e, margin %.2e" % (ci, _rel(out["fill_fvals"], ref["fill_fvals"]), min(margin)))
    assert list(out["fill_order"]) == list(ref["fill_order"])
    assert _rel(out["fill_fvals"], ref["fill_fvals"]) <= TOL_FILL
    np.testing.assert_allclose(out["widths_default"], ref["widths_default"], rtol=1e-12)
    for s, r in enumerate(ref["runs"]):
        it = r["iterations"]
        print("  start %d: it %d/%d fc %d/%d flag %d/%d  x err %.2e  f err %.2e" % (
            s, out["iterations"][s], it, out["funccount"][s], r["funccount"], out["exitflag"][s], r["exitflag"],
            _rel(out["hist_x"][s, :min(it, out["iterations"][s])], np.array(r["hist_x"])[:out["iterations"][s]]) if it else 0.0,
            _rel(out["hist_f"][s, :min(it, out["iterations"][s])], np.array(r["hist_f"])[:out["iterations"][s]]) if it else 0.0))
        assert out["iterations"][s] == it and out["funccount"][s] == r["funccount"] and out["exitflag"][s] == r["exitflag"]
        assert list(out["hist_k"][s, :it]) == list(r["hist_k"])                      # the same accepted candidates
        assert it >= 3 or c["h0"].size <= 64      # Nhyp > 64: the third direction is the first that is a full H product (the CPU test shows it is one)
        if it:
            assert _rel(out["hist_x"][s, :it], np.array(r["hist_x"])) <= TOL_GRAD
            assert _rel(out["hist_f"][s, :it], np.array(r["hist_f"])) <= TOL_GRAD
        assert _rel(out["hyp"][:, s], r["x"]) <= TOL_GRAD and _rel(out["nll"][s], r["f"]) <= TOL_GRAD
        fixed = c["LB"] == c["UB"]
        assert np.all(out["hyp"][fixed, s] == c["LB"][fixed])
    assert out["best"] == ref["best"] and _rel(out["hyp_start"], ref["hyp_start"]) <= TOL_GRAD


@pytest.mark.parametrize("ci", WIDE_CASES)
def test_recorded_values_are_the_oracles_at_the_recorded_points(ci):
    """Independent of the trajectory: every value the optimiser recorded at the wide cases is the ORACLE's gplite_nlZ (with the
    case's hyper-prior) at the point recorded with it, within tests/test_gpu_nlz.py's bound for nlZ against the oracle.  That pins
    the device's own noise vector, Cholesky branch and hyper-prior (gpobj_emit) at N = 300 and 565, Nhyp = 66 and sixteen starts."""
    from oracle import vbmc_ref as R

    c, _, out = _optimized(ci)
    worst = 0.0
    for s in range(out["hyp"].shape[1]):
        assert out["iterations"][s] >= 1
        pts = [(out["hist_x"][s, k], out["hist_f"][s, k]) for k in range(out["iterations"][s])] + [(out["hyp"][:, s], out["nll"][s])]
        for x, f in pts:
            r = float(R.gplite_nlZ(x, c["gp"], c["hprior"], compute_grad=False)[0])
            worst = max(worst, abs(f - r) / max(1.0, abs(r)))
            assert abs(f - r) <= 1e-10 * max(1.0, abs(r)), (s, f, r)
    print("case %d: recorded values against the oracle %.2e" % (ci, worst))


def test_speculation_width_does_not_change_a_bit():
    import vbmc_amd as va

    c = gp_case(14, D=2, N=30, meanfun=4, noisefun=(1, 0, 1), prior="mixed", infbound=2)
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], 24, seed=3)
    outs = [va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"],
                                     {"Design": design, "Nopts": 2, "TolFun": 1e-4, "W": W, "History": 128}) for W in (1, 2, 4, 8)]
    print("performed:", [o["performed"] for o in outs], "funccount:", outs[0]["funccount"])
    for o in outs[1:]:
        for k in ("hyp", "nll", "iterations", "funccount", "exitflag", "hist_x", "hist_f", "hist_k", "hyp_start", "fill_fvals"):
            assert np.array_equal(np.asarray(o[k]), np.asarray(outs[0][k])), k
    perf = [o["performed"] for o in outs]
    assert perf[0] >= int(np.sum(outs[0]["funccount"])) and all(b > a for a, b in zip(perf, perf[1:])), perf


@pytest.mark.parametrize("ci,capped", [(0, True), (2, True), (5, False)])
def test_first_order_condition_or_the_exit_flag_says_why(ci, capped):
    """capped: 15 iterations at most, every start may end with exit flag 0.  The uncapped case is parity case 5 with its own design
    and TolFun, whose second start the restatement ends with exit flag 1: there the projected gradient is checked against TolFun."""
    import vbmc_amd as va

    c, ptol, _ = parity_case(ci)
    tol = 1e-5 if capped else ptol
    if capped:
        opts = {"Ninit": 32, "Nopts": 3, "TolFun": tol, "seed": 1, "MaxIter": 15}
    else:
        design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], PARITY_NINIT, seed=3)
        opts = {"Design": design, "Nopts": PARITY_NOPTS, "TolFun": tol}
    out = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], opts)
    fun = _device_fun(va, c)
    flags = set()
    for s in range(opts["Nopts"]):
        x = out["hyp"][:, s]
        f, g = fun(x)
        pg = np.max(np.abs(x - np.clip(x - g, c["LB"], c["UB"])))
        print("start %d: flag %d it %d pg %.3e nll %.10g" % (s, out["exitflag"][s], out["iterations"][s], pg, f))
        assert abs(f - out["nll"][s]) <= TOL_GRAD * max(1.0, abs(f))
        assert np.all(x >= c["LB"]) and np.all(x <= c["UB"])
        if out["exitflag"][s] == T.EXIT_GRAD:
            assert pg <= tol * (1 + 1e-6)
        else:
            assert out["exitflag"][s] in (T.EXIT_LIMIT, T.EXIT_DF, T.EXIT_STEP, T.EXIT_LINESEARCH)
            if out["exitflag"][s] == T.EXIT_LIMIT:
                assert capped and out["iterations"][s] == 15
        flags.add(int(out["exitflag"][s]))
    if not capped:
        assert T.EXIT_GRAD in flags, flags
    assert out["nll"][out["best"]] == np.nanmin(out["nll"])


def test_failed_factorisations_and_refusals():
    import vbmc_amd as va

    c = gp_case(21, D=2, N=30, meanfun=1, noisefun=(1, 0, 0), prior="flat")
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], None, 12, seed=5)
    design[[3, 7], 2] = 400.0                          # a signal variance of exp(800): no jitter makes that matrix positive definite
    out = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], None, {"Design": design, "Nopts": 2, "TolFun": 1e-3})
    assert np.isnan(out["fill_fvals"][-2:]).all() and np.isfinite(out["fill_fvals"][:-2]).all()
    assert sorted(out["fill_order"][-2:]) == [3, 7] and list(out["fill_order"][-2:]) == [3, 7]
    assert np.all(np.isfinite(out["nll"]))
    # refusals leave the context usable
    for bad in ({"Nopts": 17}, {"Nopts": 0}, {"W": 17}):
        with pytest.raises(va._lib.VbmcHipError):
            va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], None, dict({"Design": design, "Nopts": 2}, **bad))
    gp2 = dict(c["gp"], meanfun=2)
    with pytest.raises(va._lib.VbmcUnsupported):
        va.gplite_train_optimize(gp2, c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], None, {"Design": design, "Nopts": 2})
    again = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], None, {"Design": design, "Nopts": 2, "TolFun": 1e-3})
    assert np.array_equal(again["hyp"], out["hyp"]) and np.array_equal(again["fill_fvals"], out["fill_fvals"], equal_nan=True)


@pytest.mark.parametrize("bad", [(260, 299), (10, 299)], ids=["rows260_299", "rows10_299"])
def test_failed_factorisations_in_the_ragged_second_fill_chunk(bad):
    """300 rows: chunks of 256 and 44.  Rows 260 and 299 (the last) carry the hopeless signal variance, so the failure index that
    k_topt_fill_collect reads lies behind the SECOND chunk's own 44 values; with rows 10 and 299 the first chunk leaves a failure
    index behind where a second chunk that read the first one's layout would find it (and call row 266 failed).  The two NaNs sort
    last in index order, every other fill value is finite and the restatement's (driven by the device's gplite_nlZ; its decisions
    and fill gaps asserted 1e-6 from flipping as in the parity test: the smallest gap is 1.6e-3 with the oracle on the CPU)."""
    import vbmc_amd as va

    c = gp_case(21, D=2, N=30, meanfun=1, noisefun=(1, 0, 0), prior="flat")
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], None, 300, seed=5)
    design[list(bad), 2] = 400.0
    out = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], None,
                                   {"Design": design, "Nopts": 2, "TolFun": 1e-3, "MaxIter": 2, "W": 2, "History": 8})
    margin = []
    ref = T.train_optimize(_device_fun(va, c), design, 2, c["gp"]["Ncov"], c["gp"]["Nnoise"], c["LB"], c["UB"], 1e-3, MaxIter=2, margin=margin)
    assert min(margin) > 1e-6 and np.min(np.diff(ref["fill_fvals"][:-2])) > 1e-6
    print("later-chunk failures: fill err %.2e" % _rel(out["fill_fvals"][:-2], ref["fill_fvals"][:-2]))
    assert np.isnan(out["fill_fvals"][-2:]).all() and np.isfinite(out["fill_fvals"][:-2]).all()
    assert list(out["fill_order"][-2:]) == list(bad)
    assert list(out["fill_order"]) == list(ref["fill_order"])
    assert _rel(out["fill_fvals"][:-2], ref["fill_fvals"][:-2]) <= TOL_FILL
    np.testing.assert_allclose(out["widths_default"], ref["widths_default"], rtol=1e-12)
    assert np.all(np.isfinite(out["nll"]))
    for s, r in enumerate(ref["runs"]):
        assert out["iterations"][s] == r["iterations"] and list(out["hist_k"][s, :r["iterations"]]) == list(r["hist_k"])
        assert _rel(out["hyp"][:, s], r["x"]) <= TOL_GRAD and _rel(out["nll"][s], r["f"]) <= TOL_GRAD


def test_candidate_that_needs_the_jitter_retries_takes_the_stall_path():
    """Three duplicated training inputs and a start at a noise of 1e-8 (variance 1e-16, below the rounding of the kernel matrix's
    diagonal): the unjittered factorisation of the start fails, the chain stalls and the host repeats the round with the x10
    retries.  With W = 1 every stall shows as one evaluation launched twice: performed > funccount.  Ninit = 0: the branch of
    gplite_train.m:249-256 (the given column is the start)."""
    import vbmc_amd as va

    c = gp_case(31, D=2, N=30, meanfun=0, noisefun=(1, 0, 0), prior="flat")
    gp = dict(c["gp"])
    X, y = gp["X"].copy(), gp["y"].copy()
    X[1], X[2], y[1], y[2] = X[0], X[0], y[0], y[0]
    gp["X"], gp["y"] = X, y
    LB, UB, h0 = c["LB"].copy(), c["UB"].copy(), c["h0"].copy()
    LB[3], h0[3] = np.log(1e-9), np.log(1e-8)
    h0[2] = max(h0[2], 0.5)                            # signal variance > 1: a noise variance of 1e-16 is below its rounding
    UB[2] = max(UB[2], 1.0)
    cc = dict(c, gp=gp)
    out = va.gplite_train_optimize(gp, h0, LB, UB, None, None, None, {"Ninit": 0, "Nopts": 1, "TolFun": 1e-4, "W": 1, "History": 64, "MaxIter": 40})
    ref = T.train_optimize(_device_fun(va, cc), h0[None], 1, 3, 1, LB, UB, 1e-4, MaxIter=40, fill=False)
    r = ref["runs"][0]
    print("stall: performed %d funccount %d it %d flag %d; ref fc %d it %d flag %d; fill %r" % (
        out["performed"], out["funccount"][0], out["iterations"][0], out["exitflag"][0], r["funccount"], r["iterations"], r["exitflag"], out["fill_fvals"]))
    assert out["performed"] > out["funccount"][0]
    # the stalled and repeated rounds leave the sequential algorithm's trajectory as it is
    assert out["iterations"][0] == r["iterations"] and out["funccount"][0] == r["funccount"] and out["exitflag"][0] == r["exitflag"]
    assert list(out["hist_k"][0, :r["iterations"]]) == list(r["hist_k"])
    assert _rel(out["hyp"][:, 0], r["x"]) <= TOL_GRAD and _rel(out["nll"][0], r["f"]) <= TOL_GRAD
    assert np.isfinite(out["fill_fvals"][0]) and _rel(out["fill_fvals"], ref["fill_fvals"]) <= TOL_FILL
    assert np.isfinite(out["nll"][0]) and out["nll"][0] <= out["fill_fvals"][0]
    np.testing.assert_allclose(out["widths_default"], UB - LB)


# ---- the reference's known answers with gplite_train in the place of the scipy stand-in -------------------------------------------
TOLERR = (0.5, 0.5)              # test/runtest_vbmc.m:9


@pytest.mark.parametrize("D,noisy,Ns", [(6, False, 0), (3, True, 0), (3, True, 6)])
def test_reference_known_answers_with_gplite_train(D, noisy, Ns):
    import vbmc_amd as va
    from tests.test_gpu_known_answers import target

    rng = np.random.default_rng(12)
    sd = np.arange(1, D + 1, dtype=np.float64)
    n_post, n_box = (150, 50) if noisy else (100, 50)
    X = np.concatenate([rng.standard_normal((n_post, D)) * 1.2 * sd, rng.uniform(-2 * D, 2 * D, size=(n_box, D)), -np.ones((1, D))], axis=0)
    y = target(X)
    s2, noisefun = None, (1, 0, 0)
    if noisy:
        y = y + rng.standard_normal(y.size)
        s2, noisefun = np.ones(y.size), (1, 1, 0)
    # the box of tests/test_gpu_known_answers.py::fit_gp
    h0 = np.concatenate([np.log(np.std(X, axis=0)), [np.log(np.std(y))], [np.log(1e-2)], [np.max(y)], np.mean(X, axis=0), np.log(np.std(X, axis=0))])
    lb = np.concatenate([h0[:D] - 4, [h0[D] - 6], [np.log(1e-4)], [np.max(y) - 10 * np.ptp(y)], np.min(X, axis=0), h0[D + 3 + D:] - 3])
    ub = np.concatenate([h0[:D] + 4, [h0[D] + 6], [np.log(2.0)], [np.max(y) + 10 * np.ptp(y)], np.max(X, axis=0), h0[D + 3 + D:] + 3])
    plb, pub = h0 - 0.25 * (h0 - lb), h0 + 0.25 * (ub - h0)
    gp, hyp, output = va.gplite_train(h0, Ns, X, y, 1, 4, noisefun, s2, None, {"Ninit": 256, "Nopts": 2, "Thin": 2, "seed": 4},
                                      LB=lb, UB=ub, PLB=plb, PUB=pub)
    assert hyp.shape == (h0.size, max(Ns, 1))
    print("gplite_train: nll", output["optimize"]["nll"], "flags", output["optimize"]["exitflag"], "it", output["optimize"]["iterations"])
    K = 2
    order = np.argsort(-y)
    vp = va.make_vp(X[order[:K]].T.copy(), np.full(K, 1e-3 ** (1.0 / D) * 1.0 + 0.3), np.std(X[order[:50]], axis=0) / np.sqrt(np.mean(np.var(X[order[:50]], axis=0))) * 1.0)
    vp["w"] = np.full(K, 1.0 / K)
    lam = np.asarray(vp["lambda"], dtype=np.float64)
    vp["lambda"] = lam * np.sqrt(D / np.sum(lam ** 2))
    opts = {"MaxIterStochastic": 600}
    for it in range(3):
        vp, _, _ = va.vpoptimize_vbmc(30 if it == 0 else 10, 2 if it == 0 else 1, vp, gp, options=opts, rng=np.random.default_rng(it), seed=20 + it)
    st = vp["stats"]
    vmu = np.asarray(vp["mu"]).reshape(D, -1) @ np.asarray(vp["w"]).reshape(-1)
    err = (abs(st["elbo"] - 0.0), float(np.sqrt(np.mean((vmu - 0.0) ** 2))))
    print("known answers: |elbo - lnZ| %.3f  rmse %.3f" % err)
    assert err[0] < TOLERR[0] and err[1] < TOLERR[1], (err, st["elbo"], st["elbo_sd"], vmu)

"""GPU parity with vp.delta != 0 (misc/gplogjoint.m:164,171-172,274,313): every launch form of the expected log joint and of its
variance, against the oracle fed the same per-dimension delta.  VBMC sets vp.delta from options.Bandwidth (vpsieve_vbmc.m:16) and
the library reports delta_ok = 1, so a nonzero delta reaches the device.

Every case first asserts, through vbmc_ctx_last_launch, that the intended kernels ran (a forced form can fall back silently), and
that the case's delta matters: the oracle's outputs with and without it differ by at least 1e4 times the tolerance of each compared
quantity, so that a kernel ignoring delta cannot pass by accident.  Tolerances as tests/test_gpu_standalone.py and
tests/test_gpu_variance.py: values 1e-10, gradients 1e-9 per block, varG 1e-7 and dvarG 1e-6 of the term scale."""
import os

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._cases import (block_relerr, delta_golden_cases, load_delta_golden, relerr, synth_problem, theta_from_inputs)
from tests.test_var_restatement import check_entries

pytestmark = pytest.mark.gpu

RT_VAL, RT_GRAD, RT_VAR, RT_DVAR = 1e-10, 1e-9, 1e-7, 1e-6
MATTERS = 1e4


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


class env:
    """the library reads its launch switches with getenv per call: set for the duration of a block"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def problem(seed, D, N, K, S, meanfun, scalar=False):
    p = synth_problem(seed, D, N, K, S, meanfun=meanfun)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=meanfun)
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    rng = np.random.default_rng(1000 + seed)
    # of the order of ell_d (~0.8) and sigma_k lambda_d: z moves by O(1); the entries differ per dimension.  Smaller beyond D = 16: z is
    # a product over the dimensions, and a delta that shrinks it by orders leaves I_k ~ m0 and the eta gradient a cancellation (D = 32
    # at full size: dG_eta ~ 3e-7 against I_k ~ 60, below fp64 resolution at 1e-9 in either the oracle or the device)
    vp["delta"] = 0.7 if scalar else (0.5 + 0.8 * rng.random(D)) * min(1.0, 16.0 / D)
    theta = np.concatenate([p["mu"].reshape(-1, order="F"), np.log(p["sigma"]), np.log(p["lam"]), p["eta"]])
    return p, gp, vp, theta


def no_delta(vp):
    return dict(vp, delta=None)


def forms(va):
    return va.default_engine().ctx.last_launch()


def matters(with_delta, without, tol, scale=None):
    """the case's delta moves the quantity by >= 1e4 x its tolerance"""
    assert relerr(without, with_delta, scale) >= MATTERS * tol, (relerr(without, with_delta, scale), tol)


def grad_ok(got, ref, D, K, tol=RT_GRAD):
    err = block_relerr(got, ref, D, K)
    assert max(err.values()) < tol, err


def mc_case(va, seed, D, N, K, S, meanfun, Ns, ent_form, lj_form, **switches):
    """negelcbo with the Monte-Carlo entropy and its gradient, the caller's draws: the forms that carry the log joint as a role"""
    p, gp, vp, theta = problem(seed, D, N, K, S, meanfun)
    eps = np.random.default_rng(seed).standard_normal((K, (Ns + 1) // 2, D))
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    ref0 = R.negelcbo_vbmc(theta, 0, no_delta(vp), gp, Ns, True, 0, eps=eps)
    matters(ref["G"], ref0["G"], RT_VAL)
    matters(ref["dG"], ref0["dG"], RT_GRAD)
    with env(**switches):
        r = va.negelcbo_batch(theta, 0, vp, gp, Ns, True, 0, eps=eps)
        assert forms(va) == (ent_form, lj_form), forms(va)
    assert relerr(r["G"][0], ref["G"]) < RT_VAL and relerr(r["F"][0], ref["F"]) < RT_VAL
    grad_ok(r["dG"][:, 0], ref["dG"], D, K)
    grad_ok(r["dF"][:, 0], ref["dF"], D, K)


def lane_role_fits(D, K, N, S):
    """vbmc_amd/csrc/elbo_launch_plan.h: the role's staged inputs within 48 KB of the lane launch's dynamic LDS"""
    return (((N + 63) // 64) * 64 * (D + 4) + S * (3 * D + 2) + (D * K + 4 * K + 2 * D + 2) + D) * 8 <= 48 * 1024


# ---------------------------------------------------------------- the log-joint forms
LANE_SHAPES = [
    # D, N, K, S, meanfun, Ns
    (6, 80, 10, 3, 4, 300),
    (1, 30, 5, 2, 1, 130),      # D = 1
    (3, 50, 16, 2, 0, 200),
    (4, 704, 3, 2, 4, 90),      # lane_role_fits just holds: N = 705 would not (checked below)
]


@pytest.mark.parametrize("D,N,K,S,meanfun,Ns", LANE_SHAPES)
def test_lane_role(va, D, N, K, S, meanfun, Ns):
    from vbmc_amd import _lib

    mc_case(va, 40 + D, D, N, K, S, meanfun, Ns, _lib.ENTFORM_LANE, _lib.LJFORM_ROLE_LANE, VBMC_ENT_KERNEL="lane")


def test_lane_role_limit_is_the_librarys():
    assert lane_role_fits(4, 3, 704, 2) and not lane_role_fits(4, 3, 705, 2)


@pytest.mark.parametrize("meanfun", [0, 1, 4])
def test_lane_role_off_runs_the_separate_kernel(va, meanfun):
    from vbmc_amd import _lib

    # VBMC_LJ_CO=0: the same lane entropy launch, the log joint on its own (split: N > 64 on a single chain)
    mc_case(va, 50 + meanfun, 5, 90, 8, 2, meanfun, 150, _lib.ENTFORM_LANE, _lib.LJFORM_VALU_SPLIT, VBMC_ENT_KERNEL="lane", VBMC_LJ_CO="0")
    # ... and a training set beyond the role's LDS block falls back to it by itself
    mc_case(va, 60 + meanfun, 4, 705, 3, 2, meanfun, 90, _lib.ENTFORM_LANE, _lib.LJFORM_VALU_SPLIT, VBMC_ENT_KERNEL="lane")


MFMA_ROLE_SHAPES = [
    (5, 60, 20, 2, 4, 100),     # K > 16
    (14, 50, 8, 1, 0, 64),      # D > 12
    (3, 40, 24, 3, 1, 90),
]


@pytest.mark.parametrize("D,N,K,S,meanfun,Ns", MFMA_ROLE_SHAPES)
def test_role_in_the_matrix_core_entropy_launch(va, D, N, K, S, meanfun, Ns):
    from vbmc_amd import _lib

    mc_case(va, 70 + D, D, N, K, S, meanfun, Ns, _lib.ENTFORM_MFMA, _lib.LJFORM_ROLE_MFMA)


MFMA_LJ_SHAPES = [
    (4, 40, 6, 3, 4),
    (17, 50, 5, 2, 0),          # DT padding
    (32, 60, 4, 2, 1),
    (6, 70, 20, 2, 4),
]


@pytest.mark.parametrize("D,N,K,S,meanfun", MFMA_LJ_SHAPES)
def test_matrix_core_log_joint_with_gradient(va, D, N, K, S, meanfun):
    """gplogjoint on its own (Ns = 0: k_entlb beside it), VBMC_LJ_KERNEL=mfma: k_logjoint_mfma<DT, true>"""
    from vbmc_amd import _lib

    p, gp, vp, theta = problem(80 + D, D, N, K, S, meanfun)
    ref = R.gplogjoint(vp, gp, (1, 1, 1, 1), True, True, 0)
    ref0 = R.gplogjoint(no_delta(vp), gp, (1, 1, 1, 1), True, True, 0)
    matters(ref["F"], ref0["F"], RT_VAL)
    matters(ref["dF"], ref0["dF"], RT_GRAD)
    with env(VBMC_LJ_KERNEL="mfma"):
        F, dF = va.gplogjoint(vp, gp, (1, 1, 1, 1), nargout=2)
        assert forms(va) == (_lib.ENTFORM_LB, _lib.LJFORM_MFMA_GRAD), forms(va)
    assert relerr(F, ref["F"]) < RT_VAL
    grad_ok(dF, np.asarray(ref["dF"]).reshape(-1), D, K)


@pytest.mark.parametrize("meanfun", [0, 1, 4])
def test_matrix_core_log_joint_value_only(va, meanfun):
    """the sieve's value-only pass: S R >= 4 x 256 cells -> k_logjoint_mfma<DT, false> by the library's own choice"""
    from vbmc_amd import _lib

    D, N, K, S, Rn = 5, 60, 6, 8, 128
    p, gp, vp, theta = problem(90 + meanfun, D, N, K, S, meanfun)
    th = np.asfortranarray(theta[:, None] + 0.1 * np.random.default_rng(3).standard_normal((theta.size, Rn)))
    cols = list(range(0, Rn, 9)) + [Rn - 1]
    G = np.array([R.negelcbo_vbmc(th[:, c], 0, vp, gp, 0, False, 0)["G"] for c in cols])
    G0 = np.array([R.negelcbo_vbmc(th[:, c], 0, no_delta(vp), gp, 0, False, 0)["G"] for c in cols])
    matters(G, G0, RT_VAL)
    r = va.negelcbo_batch(th, 0, vp, gp, 0, False, 0)
    assert forms(va) == (_lib.ENTFORM_LB, _lib.LJFORM_MFMA_VALUE), forms(va)
    assert relerr(r["G"][cols], G) < RT_VAL


@pytest.mark.parametrize("meanfun", [0, 1, 4])
@pytest.mark.parametrize("wide", [False, True])
def test_valu_log_joint_split_and_one_wave(va, meanfun, wide):
    """VBMC_LJ_KERNEL=valu with the deterministic entropy (Ns = 0, k_entlb): four waves per cell on a small grid (N > 64), one wave per
    cell once ((K + 3) / 4) S R >= 8 x 256; several restarts in one pass, each against its own oracle"""
    from vbmc_amd import _lib

    D, N, K, S = 4, 90, 16, 8
    Rn = 64 if wide else 3
    p, gp, vp, theta = problem(100 + meanfun, D, N, K, S, meanfun)
    th = np.asfortranarray(theta[:, None] + 0.1 * np.random.default_rng(4).standard_normal((theta.size, Rn)))
    cols = (0, Rn // 2, Rn - 1)
    refs = [R.negelcbo_vbmc(th[:, c], 0, vp, gp, 0, True, 0) for c in cols]
    for c, ref in zip(cols, refs):
        ref0 = R.negelcbo_vbmc(th[:, c], 0, no_delta(vp), gp, 0, True, 0)
        matters(ref["G"], ref0["G"], RT_VAL)
        matters(ref["dG"], ref0["dG"], RT_GRAD)
    with env(VBMC_LJ_KERNEL="valu"):
        r = va.negelcbo_batch(th, 0, vp, gp, 0, True, 0)
        assert forms(va) == (_lib.ENTFORM_LB, _lib.LJFORM_VALU_WAVE if wide else _lib.LJFORM_VALU_SPLIT), forms(va)
    for c, ref in zip(cols, refs):
        assert relerr(r["F"][c], ref["F"]) < RT_VAL and relerr(r["G"][c], ref["G"]) < RT_VAL and relerr(r["H"][c], ref["H"]) < RT_VAL
        grad_ok(r["dG"][:, c], ref["dG"], D, K)
        grad_ok(r["dF"][:, c], ref["dF"], D, K)


# ---------------------------------------------------------------- the variance forms
@pytest.mark.parametrize("meanfun", [0, 1, 4])
@pytest.mark.parametrize("low_noise", [False, True])
def test_full_variance_and_separate_K(va, meanfun, low_noise):
    """compute_var = 1 with separate_K (k_var_z, k_tri_gemm or the substitution, k_var_gram_mfma): I_sk, J_sjk, varG; low_noise: two
    hyper-samples in the Lchol = false representation (k_symm, gplite_core.m:98)"""
    D, N, K, S = 4, 50, 6, 3
    p, gp, vp, theta = problem(110 + meanfun, D, N, K, S, meanfun)
    if low_noise:
        for s in (0, 2):
            post = gp["post"][s]
            sl = 1.0 / post["sW"][0] ** 2
            post["L"] = -R.solve_upper(post["L"], R.solve_upper_t(post["L"], np.eye(N))) / sl
            post["Lchol"] = False
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, 0, False, 1, separate_K=True)
    ref0 = R.negelcbo_vbmc(theta, 0, no_delta(vp), gp, 0, False, 1, separate_K=True)
    scale = max(1.0, np.max(np.abs(ref["J_sjk"])))
    matters(ref["I_sk"], ref0["I_sk"], RT_VAL)
    matters(ref["J_sjk"], ref0["J_sjk"], RT_VAR, scale)
    matters(ref["varG"], ref0["varG"], RT_VAR, max(1.0, abs(ref["varG"]), scale))
    out = va.negelcbo_vbmc(theta, 0, vp, gp, 0, 0, 1, nargout=11)
    assert relerr(out[2], ref["G"]) < RT_VAL and relerr(out[9], ref["I_sk"]) < RT_VAL
    assert np.max(np.abs(out[10] - ref["J_sjk"])) < RT_VAR * scale
    assert abs(out[7] - ref["varG"]) < RT_VAR * max(1.0, abs(ref["varG"]), scale)
    assert abs(out[6] - ref["varGss"]) < RT_VAR * max(1.0, abs(ref["varGss"]), scale)
    check_entries(gp, vp, 1, what="delta, full", J=out[10], varG=out[7], varGss=out[6])     # per entry (tests/_var_ref.py)


@pytest.mark.parametrize("meanfun", [0, 1, 4])
@pytest.mark.parametrize("low_noise", [False, True])
def test_diag_variance_and_its_gradient(va, meanfun, low_noise):
    """compute_var = 2 with its gradient (k_var_gram, k_vargrad, k_var_sample, k_var_final): gplogjoint's varF / dvarF averaged and
    per hyper-sample (avg_flag = 0)"""
    from vbmc_amd import _lib

    D, N, K, S = 5, 60, 7, 3
    p, gp, vp, theta = problem(120 + meanfun, D, N, K, S, meanfun)
    if low_noise:
        post = gp["post"][1]
        sl = 1.0 / post["sW"][0] ** 2
        post["L"] = -R.solve_upper(post["L"], R.solve_upper_t(post["L"], np.eye(N))) / sl
        post["Lchol"] = False
    for avg in (True, False):
        ref = R.gplogjoint(vp, gp, (1, 1, 1, 1), avg, True, 2, compute_vargrad=True)
        ref0 = R.gplogjoint(no_delta(vp), gp, (1, 1, 1, 1), avg, True, 2, compute_vargrad=True)
        vsc = max(1.0, np.max(np.abs(ref["varF"])))
        dsc = max(1.0, np.max(np.abs(ref["dvarF"])))
        matters(ref["F"], ref0["F"], RT_VAL)
        matters(ref["varF"], ref0["varF"], RT_VAR, vsc)
        matters(ref["dvarF"], ref0["dvarF"], RT_DVAR, dsc)
        F, dF, varF, dvarF = va.gplogjoint(vp, gp, (1, 1, 1, 1), avg, True, 2, nargout=4)
        assert forms(va)[1] in (_lib.LJFORM_VALU_WAVE, _lib.LJFORM_MFMA_GRAD), forms(va)
        assert relerr(F, ref["F"]) < RT_VAL
        dF, rdF = np.asarray(dF).reshape(-1, 1 if avg else S), np.asarray(ref["dF"]).reshape(-1, 1 if avg else S)
        for s in range(dF.shape[1]):
            grad_ok(dF[:, s], rdF[:, s], D, K)
        assert relerr(varF, ref["varF"], vsc) < RT_VAR
        assert relerr(dvarF, np.asarray(ref["dvarF"]).reshape(np.shape(dvarF)), dsc) < RT_DVAR
        check_entries(gp, vp, 2, (1, 1, 1, 1), what="delta, diagonal", **(dict(varG=varF, dvarF=dvarF) if avg else dict(varF_s=varF, dvarF_s=dvarF)))


# ---------------------------------------------------------------- call paths
def test_pipelined_passes_with_and_without_delta(va):
    """two evaluations in flight on different slots, one with delta and one without: each matches its own oracle (crosstalk through
    the staging buffers -- the H2D block carries delta^2 -- would show)"""
    D, N, K, S, Rn, Ns = 5, 50, 6, 2, 3, 0
    p, gp, vp, theta = problem(130, D, N, K, S, 4)
    th = np.asfortranarray(theta[:, None] + 0.1 * np.random.default_rng(5).standard_normal((theta.size, Rn)))
    T = theta.size
    po_d = va.PreparedObjective(T, Rn, 0.0, vp, gp, Ns)
    po_0 = va.PreparedObjective(T, Rn, 0.0, no_delta(vp), gp, Ns)
    from vbmc_amd import _lib

    for _ in range(2):
        po_d.submit(th, slot=0)
        assert forms(va) == (_lib.ENTFORM_LB, _lib.LJFORM_VALU_WAVE), forms(va)
        po_0.submit(th, slot=1)
        F0, dF0 = [x.copy() for x in po_0.collect(1)]
        Fd, dFd = [x.copy() for x in po_d.collect(0)]
        for c in range(Rn):
            ref = R.negelcbo_vbmc(th[:, c], 0, vp, gp, Ns, True, 0)
            ref0 = R.negelcbo_vbmc(th[:, c], 0, no_delta(vp), gp, Ns, True, 0)
            matters(ref["F"], ref0["F"], RT_VAL)
            assert relerr(Fd[c], ref["F"]) < RT_VAL and relerr(F0[c], ref0["F"]) < RT_VAL
            grad_ok(dFd[:, c], ref["dF"], D, K)
            grad_ok(dF0[:, c], ref0["dF"], D, K)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_over_hyper_samples(va, world):
    """the S-sharded evaluation (tests/test_gpu_shard_s.py's one-process harness) with delta: bit-identical to the unsharded pass with
    the same chunking, and the oracle's numbers"""
    from tests.test_gpu_shard_s import _sharded

    D, N, K, S = 4, 60, 5, 3
    p, gp, vp, theta = problem(140, D, N, K, S, 4)
    th = np.asfortranarray(theta[:, None])
    from vbmc_amd import _lib

    got = _sharded(va, world, th, vp, gp, 0, None, 7)
    assert forms(va) == (_lib.ENTFORM_LB, _lib.LJFORM_VALU_WAVE), forms(va)      # (the ranks' passes: one hyper-sample each, N <= 64)
    one = va.negelcbo_batch(th, 0, vp, gp, 0, True, 0, None, seed=7, chunk_world=world)
    for k in ("F", "G", "H", "dF", "dG", "dH"):
        assert np.array_equal(got[k], one[k]), k
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, 0, True, 0)
    ref0 = R.negelcbo_vbmc(theta, 0, no_delta(vp), gp, 0, True, 0)
    matters(ref["F"], ref0["F"], RT_VAL)
    assert relerr(got["F"][0], ref["F"]) < RT_VAL
    grad_ok(got["dF"][:, 0], ref["dF"], D, K)


def test_device_adam_with_delta_equals_host_adam(va):
    """vbmc_adam_batch with delta: the stopping iteration and the iterates of the host Adam loop over the same device objective
    (tests/test_gpu_optimize.py::test_device_adam_equals_host_adam without delta)"""
    p, gp, vp, theta = problem(150, 4, 50, 5, 3, 4)
    opts = dict(TolLength=1e-6, TolWeight=1e-2, TolConLoss=0.01, WeightPenalty=0.1)
    vpb, tb = R.vpbounds(vp, gp, opts)
    vpb["delta"] = vp["delta"]
    Ns, seed, MaxIter = 60, 77, 200
    it = {"n": 0}

    def fun(x):
        it["n"] += 1
        r = va.negelcbo_batch(x, 0, vpb, gp, Ns, True, 0, tb, seed=seed + it["n"])
        return float(r["F"][0]), r["dF"][:, 0]

    xh, fh, xth, fth, ith = va.fminadam(fun, theta, None, None, 1e-3, MaxIter)
    host_forms = forms(va)
    xd, fd, xtd, ftd, itd = va.fminadam_device(theta, 0, vpb, gp, Ns, tb, 1e-3, MaxIter, seed=seed)
    # the device loop's passes run the kernels the host loop's calls ran
    assert forms(va) == host_forms and min(host_forms) > 0, (forms(va), host_forms)
    assert int(itd[0]) == ith
    assert relerr(ftd[0], fth) < 1e-9 and relerr(xtd[0], xth) < 1e-9
    assert relerr(xd[:, 0], xh) < 1e-9 and abs(fd[0] - fh) < 1e-9 * max(1, abs(fh))
    # the objective it minimised is the delta one: the starting point's value against the oracle
    ref = R.negelcbo_vbmc(theta, 0, vpb, gp, 0, True, 0, thetabnd=tb)
    ref0 = R.negelcbo_vbmc(theta, 0, no_delta(vpb), gp, 0, True, 0, thetabnd=tb)
    matters(ref["G"], ref0["G"], RT_VAL)
    r = va.negelcbo_batch(theta, 0, vpb, gp, 0, True, 0, tb)
    assert relerr(r["G"][0], ref["G"]) < RT_VAL


@pytest.mark.parametrize("path", delta_golden_cases())
def test_golden_delta_family_on_the_device(va, path):
    """tests/golden/mp_delta_case*.json through the device, as tests/test_gpu_elbo.py::test_golden_vectors does without delta:
    G_s, dG_s, I_sk, J_sjk, varG_s (full and diagonal) and dvarG_s against the 50-digit values"""
    inp, vp, gp, exp = load_delta_golden(path)
    S, D, K = inp["S"], inp["D"], inp["K"]
    T = D * K + 2 * K + D
    F, dF, varF, dvarF = va.gplogjoint(vp, gp, (1, 1, 1, 1), False, True, 2, nargout=4)
    assert relerr(np.atleast_1d(F), exp["G_s"]) < RT_VAL
    dF, dvarF = np.asarray(dF).reshape(T, S), np.asarray(dvarF).reshape(T, S)
    vsc = max(1.0, np.max(np.abs(exp["varG_s_diag"])))
    assert relerr(np.atleast_1d(varF), exp["varG_s_diag"], vsc) < RT_VAR
    for s in range(S):
        grad_ok(dF[:, s], exp["dG_s"][s], D, K)
        assert relerr(dvarF[:, s], exp["dvarG_s_diag"][s], max(1.0, np.max(np.abs(exp["dvarG_s_diag"])))) < RT_DVAR
    out = va.gplogjoint(vp, gp, (0, 0, 0, 0), False, True, 1, True, nargout=7)
    jsc = max(1.0, np.max(np.abs(exp["J_sjk"])))
    assert relerr(np.atleast_1d(out[2]), exp["varG_s_full"], jsc) < RT_VAR
    assert relerr(np.asarray(out[5]).reshape(S, K), exp["I_sk"]) < RT_VAL
    assert np.max(np.abs(np.asarray(out[6]).reshape(S, K, K) - exp["J_sjk"])) < RT_VAR * jsc
    check_entries(gp, vp, 2, (1, 1, 1, 1), what="golden, diagonal", varF_s=varF, dvarF_s=dvarF)
    check_entries(gp, vp, 1, what="golden, full", J=np.asarray(out[6]).reshape(S, K, K), varF_s=out[2])
    # the same family through the objective: negelcbo's G is gplogjoint's F averaged over the hyper-samples
    theta = theta_from_inputs(inp)
    r = va.negelcbo_batch(theta, 0, vp, gp, 0, True, 0)
    assert relerr(r["G"][0], np.mean(exp["G_s"])) < RT_VAL

"""The matrix-core entropy kernel's gradient with ONE PV product per antithetic pair (vbmc_amd/csrc/entropy_mfma.h: PM, ent_pm_for).  With
r+-_ik = n+-_ik / q'+-_i, p = r+ + r-, m = r+ - r-, a_k = w_k / sigma_k^2 and V_kd = a_k m'_kd the two signs' pieces add up to

    W_k  = sum_i p_ik
    G_d  = sum_i u'_id Am_i - sum_k V_kd W_k        Am_i = sum_k a_k m_ik
    LG_d = sum_i u'_id (u'_id Ap_i - Bm_id)         Ap_i = sum_k a_k p_ik,  Bm_id = sum_k V_kd m_ik

(test_regrouped_pair_formulas_equal_the_per_sign_formulas restates both forms in numpy).  The mu-gradient is then a difference of two sums,
the second one formed in the wave's epilogue from the finished weight record -- so every test here runs on a mixture whose components
OVERLAP (sigma x 6): on the well separated mixtures of tests/_cases.py the mu-block of dH is cancellation noise below block_relerr's floor
and a wrong epilogue coefficient would not show.  Each test asserts the condition on its reference: the mu-block is at least 1e-3 of dH's
largest entry.

Three k-tiles with a one-value tail at D = 7..10 (K = 49..52) take the form; three k-tiles without a tail (K = 41..48) keep the sample
layout's per-sign form (their registers decide, see ent_pm_for), and the matrix holds both to the same bounds: the project's RT_VAL / RT_GRAD
per block against the oracle on the dumped device stream; 1e-13 / 1e-12 between two device kernels on the same draws, where only the order
of summation differs; and the mu-block against ITS OWN largest entry at 1e-11 (the subtraction of the two sums is good to about 1e-15 at
5000 samples in numpy float64 against longdouble; a wrong coefficient is O(1))."""
import ctypes

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._cases import block_relerr, relerr
from tests.test_gpu_elbo import RT_GRAD, RT_VAL, problem

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def overlapping(seed, D, K, N=30, S=2):
    """problem(seed, D, N, K, S) with every component six times as wide, in theta and in vp alike"""
    p, gp, vp, theta = problem(seed, D, N, K, S)
    theta = theta.copy()
    theta[D * K:D * K + K] += np.log(6.0)
    vp = dict(vp)
    vp["sigma"] = np.asarray(vp["sigma"]) * 6.0
    return p, gp, vp, theta


def mu_block_counts(dH, D, K):
    """the condition every reference here has to meet: the mu-block of dH is no cancellation noise"""
    dH = np.asarray(dH).reshape(-1)
    return np.max(np.abs(dH[:D * K])) >= 1e-3 * np.max(np.abs(dH))


def blocks_ok(got, ref, D, K, tol=RT_GRAD):
    err = block_relerr(got, ref, D, K)
    assert max(err.values()) < tol, err


def assert_matrix_core_one_wave(va, D, K):
    """the pass that just ran used the matrix-core entropy kernel, and the policy's instantiation for the shape has single-wave workgroups
    and three k-tiles"""
    from vbmc_amd import _lib

    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_MFMA
    q = [ctypes.c_int() for _ in range(4)]
    kind = _lib.load().vbmc_entropy_plan(D, K, *[ctypes.byref(x) for x in q])
    assert kind == 1 and q[0].value == 3 and q[1].value == 3 and q[2].value == 1, [x.value for x in q]


# D: the places the last dimension lands in the slot map (9 and 10 share register 2 with Am).  K: third k-tile partial, no tail (the LDS
# re-read of u'), a tail of two, a tail of four.
@gpu
@pytest.mark.parametrize("K", [41, 48, 50, 52])
@pytest.mark.parametrize("D", [7, 9, 10])
def test_sign_pair_against_the_oracle_on_the_device_stream(va, D, K, monkeypatch):
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    p, gp, vp, theta = overlapping(300 + 13 * D + K, D, K)
    eng = va.default_engine()
    for Ns, seed in ((32, 11), (74, 12)):                   # Mh = 16: one full tile; Mh = 37: two full tiles and a partial one of 5
        eps = eng.ctx.rng_dump(D, K, 1, Ns, seed)[0]
        ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
        assert mu_block_counts(ref["dH"], D, K)
        out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=seed)
        assert_matrix_core_one_wave(va, D, K)
        err = dict(H=relerr(out["H"][0], ref["H"]), dH=block_relerr(out["dH"][:, 0], ref["dH"], D, K), dF=block_relerr(out["dF"][:, 0], ref["dF"], D, K))
        print("D %d K %d Ns %d: %s" % (D, K, Ns, err))
        assert err["H"] < RT_VAL
        blocks_ok(out["dH"][:, 0], ref["dH"], D, K)
        blocks_ok(out["dF"][:, 0], ref["dF"], D, K)


@gpu
@pytest.mark.parametrize("K", [41, 50])
def test_sign_pair_against_the_valu_kernel(va, K, monkeypatch):
    """k_entropy (one lane per sample, no matrix cores, the per-sign formulas) on the same device stream"""
    from vbmc_amd import _lib

    D, Ns, R_ = 10, 74, 3
    p, gp, vp, theta = overlapping(370 + K, D, K)
    thetas = theta[:, None] + 0.05 * np.random.default_rng(K).standard_normal((theta.size, R_))
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    m = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=21)
    assert_matrix_core_one_wave(va, D, K)
    monkeypatch.setenv("VBMC_ENT_KERNEL", "valu")
    v = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=21)
    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_VALU
    print("K %d: H %.2e" % (K, relerr(m["H"], v["H"])))
    assert relerr(m["H"], v["H"]) < 1e-13
    for r in range(R_):
        assert mu_block_counts(v["dH"][:, r], D, K)
        e_all, e_mu = relerr(m["dH"][:, r], v["dH"][:, r]), relerr(m["dH"][:D * K, r], v["dH"][:D * K, r])
        print("  restart %d: dH %.2e, mu-block against its own largest entry %.2e" % (r, e_all, e_mu))
        assert e_all < 1e-12
        assert e_mu < 1e-11


# ---------------------------------------------------------------- the siblings of the class, D = 10, K = 50
@pytest.fixture(scope="module")
def headline():
    return overlapping(61, 10, 50, N=80, S=20)


@gpu
def test_sign_pair_in_the_launch_that_carries_the_log_joint_role(va, headline, monkeypatch):
    from vbmc_amd import _lib

    p, gp, vp, theta = headline
    monkeypatch.delenv("VBMC_ENT_CHUNKS", raising=False)
    monkeypatch.delenv("VBMC_LJ_CO", raising=False)
    Ns, seed = 3000, 5
    eps = va.default_engine().ctx.rng_dump(10, 50, 1, Ns, seed)[0]
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    assert mu_block_counts(ref["dH"], 10, 50)
    out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=seed)
    assert va.default_engine().ctx.last_launch() == (_lib.ENTFORM_MFMA, _lib.LJFORM_ROLE_MFMA)
    assert relerr(out["H"][0], ref["H"]) < RT_VAL and relerr(out["G"][0], ref["G"]) < RT_VAL
    blocks_ok(out["dH"][:, 0], ref["dH"], 10, 50)
    blocks_ok(out["dF"][:, 0], ref["dF"], 10, 50)


@gpu
def test_sign_pair_in_parity_mode(va, headline):
    """the caller's draws: the instantiation that prefetches its tile (ten of the PV operands in registers, two in LDS -- the epilogue's
    contraction reads both)"""
    p, gp, vp, theta = headline
    D, K, Ns = 10, 50, 74
    eps = np.random.default_rng(9).standard_normal((K, Ns // 2, D))
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    assert mu_block_counts(ref["dH"], D, K)
    out = va.negelcbo_batch(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    assert_matrix_core_one_wave(va, D, K)
    assert relerr(out["H"][0], ref["H"]) < RT_VAL
    blocks_ok(out["dH"][:, 0], ref["dH"], D, K)
    blocks_ok(out["dF"][:, 0], ref["dF"], D, K)


@gpu
def test_sign_pair_chunk_grid_equals_the_walking_launch(va, monkeypatch):
    """The walking launch keeps the per-sign form with the LDS exchange (GP2): the same draws and the same exponentials, another gradient
    algebra.  A blocking call takes the walk once the chunk grid would hand every wave slot two waves -- at Ns = 200 (seven tiles, one
    chunk) that is K R >= 4096: R = 96."""
    D, K, Ns, R_ = 10, 50, 200, 96
    p, gp, vp, theta = overlapping(340, D, K)
    thetas = theta[:, None] + 0.05 * np.random.default_rng(D).standard_normal((theta.size, R_))
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    monkeypatch.delenv("VBMC_ENT_WALK", raising=False)
    w = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=77)
    monkeypatch.setenv("VBMC_ENT_WALK", "0")
    c = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=77)
    assert_matrix_core_one_wave(va, D, K)
    assert not np.array_equal(w["dH"], c["dH"]), "the walking launch did not run (same bits as the chunk grid)"
    assert relerr(w["H"], c["H"]) < 1e-13
    worst = 0.0
    for r in range(R_):
        assert mu_block_counts(w["dH"][:, r], D, K)
        worst = max(worst, relerr(c["dH"][:, r], w["dH"][:, r]))
    print("chunk grid against the walk: H %.2e, dH %.2e" % (relerr(w["H"], c["H"]), worst))
    assert worst < 1e-12


# ---------------------------------------------------------------- the derivation, executable (no GPU)
def test_regrouped_pair_formulas_equal_the_per_sign_formulas():
    """ent/entmc_vbmc.m:77-100 in the kernel's centred coordinates, for every source component j of an overlapping mixture: the per-sign
    accumulation against the regrouped one.  D = 4, K = 5, 64 base samples; each block to 1e-12 of its largest entry."""
    D, K, M = 4, 5, 64
    rng = np.random.default_rng(5)
    mu = rng.uniform(-1.0, 1.0, (K, D))
    sig = rng.uniform(0.8, 1.6, K)                   # widths of the order of the distances: every component sees every other
    w = rng.dirichlet(np.ones(K))
    a = w / sig ** 2
    for j in range(K):
        mp = mu - mu[j]                              # m'_k
        V = a[:, None] * mp                          # V_kd
        u = sig[j] * rng.standard_normal((M, D))     # u'_i

        def dens(t):                                 # n_ik up to the sample's own factor, which cancels in n / q'
            return np.exp(-0.5 * np.sum((t[:, None, :] - mp[None]) ** 2, axis=2) / sig ** 2 - D * np.log(sig))

        G1, LG1, W1 = np.zeros(D), np.zeros(D), np.zeros(K)
        r = {}
        for s in (1.0, -1.0):
            t = s * u
            n = dens(t)
            q = n @ w
            gd = (t * (n @ a)[:, None] - n @ V) / q[:, None]
            G1 += gd.sum(0)
            LG1 += (t * gd).sum(0)
            W1 += (n / q[:, None]).sum(0)
            r[s] = n / q[:, None]
        pp, mm = r[1.0] + r[-1.0], r[1.0] - r[-1.0]
        W2 = pp.sum(0)
        G2 = (u * (mm @ a)[:, None]).sum(0) - V.T @ W2
        LG2 = (u * (u * (pp @ a)[:, None] - mm @ V)).sum(0)
        assert np.max(np.abs(G1)) > 1e-3 * np.max(np.abs(LG1))      # the mixture overlaps: G is no cancellation noise
        for got, ref in ((G2, G1), (LG2, LG1), (W2, W1)):
            assert relerr(got, ref) < 1e-12

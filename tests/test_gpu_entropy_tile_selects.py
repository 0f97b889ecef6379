"""The two places of the matrix-core entropy kernel's tile loop that the compiler turns into selects (vbmc_amd/csrc/entropy_mfma.h): the
padding masks of the sample fragment ev[] and the counted renormalisation of the mantissa product (fold).  Written for a form of the loop
without them, which was measured and not kept (profiles/r08_logjoint_rows.md); the cases hold whatever form the loop has, at QS = 3
(D = 7..10), where that form was derived.

  D = 10, 9: the padding is the tail of the last dim-block (the first mask); D = 7 = 4 QS - 5: the whole last dim-block and the last slot
  of the one before (the second mask).  On the device stream the padded slots hold DRAWS, so a mask that let them through would show.
  K = 18: one k-tile + tail; K = 50: three + tail, the headline class -- with and without the log-joint role in the launch (two
  instantiations), in parity mode (draws from memory: a third) and value-only (a fourth).
  A product of more than 256 factors per wave (K = 2, one chunk per component: 256 tiles, 512 signs): the renormalisation inside the
  tile loop, after a full tile and -- Ns = 8190 -- after the partial one.

Against k_entropy (one lane per sample, no matrix cores, no shared code with the tile body) on the same device stream: H 1e-13, dH 1e-12 --
two device kernels on the same draws, where only the order of summation differs (as tests/test_gpu_entropy_sample_layout.py).  Against
the oracle: the project's RT_VAL / RT_GRAD."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._cases import relerr
from tests.test_gpu_elbo import RT_VAL, problem
from tests.test_gpu_entropy_sample_layout import assert_matrix_core_one_wave, blocks_ok

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


@pytest.mark.parametrize("K", [18, 50])
@pytest.mark.parametrize("D", [7, 9, 10])
def test_tile_loop_against_the_valu_kernel_and_the_oracle(va, D, K, monkeypatch):
    from vbmc_amd import _lib

    Ns, R_, seed = 74, 3, 21                # Mh = 37: two full tiles and a partial one of 5
    p, gp, vp, theta = problem(300 + 13 * D + K, D, 30, K, 2)
    thetas = np.asfortranarray(theta[:, None] + 0.05 * np.random.default_rng(D + K).standard_normal((theta.size, R_)))
    monkeypatch.setenv("VBMC_ENT_KERNEL", "valu")
    v = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=seed)
    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_VALU
    eps = va.default_engine().ctx.rng_dump(D, K, R_, Ns, seed)
    ref = [R.negelcbo_vbmc(thetas[:, r], 0, vp, gp, Ns, True, 0, eps=eps[r]) for r in range(R_)]
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    for co in (None, "0"):                  # the launch the plan chooses, and the one without the log-joint role
        if co is None:
            monkeypatch.delenv("VBMC_LJ_CO", raising=False)
        else:
            monkeypatch.setenv("VBMC_LJ_CO", co)
        m = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=seed)
        assert_matrix_core_one_wave(va, D, K)
        eH = relerr(m["H"], v["H"])
        eG = max(relerr(m["dH"][:, r], v["dH"][:, r]) for r in range(R_))
        print("D %d K %d role %s: H %.2e dH %.2e against the VALU kernel" % (D, K, co, eH, eG))
        assert eH < 1e-13
        assert eG < 1e-12
        for r in range(R_):
            assert relerr(m["H"][r], ref[r]["H"]) < RT_VAL
            blocks_ok(m["dH"][:, r], ref[r]["dH"], D, K)
            blocks_ok(m["dF"][:, r], ref[r]["dF"], D, K)


@pytest.mark.parametrize("D", [7, 10])
def test_tile_loop_in_parity_mode_and_value_only(va, D):
    """the caller's draws (the prefetching instantiation; padded slots are zero there, the masks must leave the dimensions alone), and the
    value-only kernel on the device stream"""
    K, Ns = 50, 74
    p, gp, vp, theta = problem(340 + D, D, 30, K, 2)
    eps = np.random.default_rng(9).standard_normal((K, Ns // 2, D))
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    d = va.negelcbo_batch(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    assert_matrix_core_one_wave(va, D, K)
    assert relerr(d["H"][0], ref["H"]) < RT_VAL
    blocks_ok(d["dH"][:, 0], ref["dH"], D, K)
    blocks_ok(d["dF"][:, 0], ref["dF"], D, K)
    seed = 33
    epsd = va.default_engine().ctx.rng_dump(D, K, 1, Ns, seed)[0]
    refv = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, False, 0, eps=epsd)
    vo = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, False, 0, seed=seed)
    assert_matrix_core_one_wave(va, D, K)
    g = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=seed)
    assert relerr(vo["H"][0], refv["H"]) < RT_VAL and relerr(vo["F"][0], refv["F"]) < RT_VAL
    assert relerr(vo["H"][0], g["H"][0]) < 1e-13           # the value-only and the gradient kernel on the same draws


@pytest.mark.parametrize("Ns", [8192, 8190])
def test_product_of_more_than_256_factors_per_wave(va, Ns, monkeypatch):
    """K = 2, one restart, ONE chunk per component: a wave multiplies 512 mantissas and renormalises after tiles 128 and 256 (Ns = 8190: the
    second time after the partial tile)"""
    from vbmc_amd import _lib

    D, K = 10, 2
    p, gp, vp, theta = problem(77, D, 30, K, 2)
    monkeypatch.setenv("VBMC_ENT_CHUNKS", "1")
    monkeypatch.setenv("VBMC_ENT_KERNEL", "valu")
    v = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=4)
    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_VALU
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    for co in (None, "0"):
        if co is None:
            monkeypatch.delenv("VBMC_LJ_CO", raising=False)
        else:
            monkeypatch.setenv("VBMC_LJ_CO", co)
        m = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=4)
        assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_MFMA
        print("Ns %d role %s: H %.2e dH %.2e" % (Ns, co, relerr(m["H"], v["H"]), relerr(m["dH"][:, 0], v["dH"][:, 0])))
        assert relerr(m["H"], v["H"]) < 1e-13
        assert relerr(m["dH"][:, 0], v["dH"][:, 0]) < 1e-12

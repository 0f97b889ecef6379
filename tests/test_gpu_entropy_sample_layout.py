"""The matrix-core entropy kernel's PV output in the SAMPLE layout (vbmc_amd/csrc/entropy_mfma.h: SL, ent_sl_for): single-wave gradient
kernels at D <= 10 run the PV MFMAs with their operands swapped, so that q', A' and B' of a sample land in the sample's own lanes
(slot s = lg + 4 r: B'_s for s < D, A' in 10, 11, q' in 12..15) and the per-sample chain needs no LDS exchange.  Not every instantiation
takes the layout (ent_sl_for: the register tables decide; sl_class below restates it): with QS = ceil((D + 2) / 4),
  QS = 3 (D = 7..10): K = 17..24 (one k-tile + tail), 37, 38 (two + a tail of eight), 41..52 (three, with or without a one-value tail; without:
                      the gradient step re-reads u' from the LDS tile, ent_sl_evl_for), 53..56 (three + a tail of eight)
  QS = 2 (D = 3..6):  K = 25..32 (two k-tiles, no tail), 41..56 (three k-tiles, any tail)
  QS = 1 (D = 1, 2):  K <= 16, 25..36, 41..48, 53..56
and everything else -- four k-tiles, D >= 11, the walking launch, value-only calls -- keeps the column layout (the parent's code).  The matrix
below is the one the layout was specified with plus the K that reach the remaining classes; test_the_matrix_runs_every_sample_layout_class
holds it to that.  Checked against the oracle on the dumped device stream at every place the last dimension can land in the slot map, on
full and partial tiles; against the independent VALU kernel; and through the siblings of the class (log-joint role, parity mode,
block-sparse mode, value-only).  Tolerances: the project's RT_VAL / RT_GRAD against the oracle; 1e-13 / 1e-12 between two device
kernels on the same draws, where only the order of summation differs (as test_walking_entropy_launch_equals_the_chunk_grid)."""
import ctypes

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._cases import block_relerr, relerr
from tests.test_gpu_elbo import RT_GRAD, RT_VAL, problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def blocks_ok(got, ref, D, K, tol=RT_GRAD):
    err = block_relerr(got, ref, D, K)
    assert max(err.values()) < tol, err


def assert_matrix_core_one_wave(va, D, K):
    """the pass that just ran used the matrix-core entropy kernel, and the policy's instantiation for the shape has single-wave workgroups.
    (The plan hook names the lane kernel's class where that one serves the shape by default -- K <= 16 -- and VBMC_ENT_KERNEL=mfma keeps
    it off: there the launch record alone says which kernel ran, and K <= 16 is one k-tile on one wave.)"""
    from vbmc_amd import _lib

    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_MFMA
    q = [ctypes.c_int() for _ in range(4)]
    kind = _lib.load().vbmc_entropy_plan(D, K, *[ctypes.byref(x) for x in q])
    assert kind in (1, 2), kind
    if kind == 1:
        assert q[2].value == 1 and q[0].value == (D + 2 + 3) // 4, [x.value for x in q]
    else:
        assert K <= 16


# D = 1..10: every place the last dimension can land in the slot map (D = 9, 10 share register 2 with A'); D = 11, 12: the first shapes that
# keep the column layout.  K: a partial k-tile, a full one, a tail of 2, a tail of 8, two and three k-tiles with tail, four k-tiles; and, for
# the classes of the layout those do not reach: two k-tiles without a tail (28), two + a tail of eight (37), three without a tail (48: at
# D >= 7 the LDS re-read of u', whose padded slots hold DRAWS on the device stream), three + a tail of eight (54).
SL_D = [1, 2, 3, 6, 7, 8, 9, 10, 11, 12]
SL_K = [3, 16, 18, 24, 34, 50, 64, 28, 37, 48, 54]


def sl_class(qs, kt, tl):
    """vbmc_amd/csrc/entropy_mfma.h: ent_sl_for for the gradient kernels of single-wave workgroups in the chunk grid, restated"""
    if qs > 3 or kt == 4:
        return False
    if qs == 3:
        return not ((kt == 1 and tl == 0) or (kt == 2 and tl <= 1))
    if qs == 2:
        return kt == 3 or (kt == 2 and tl == 0)
    return tl == 0 or (kt == 2 and tl == 1) or (kt == 3 and tl == 2)


def plan_class(D, K):
    """(qs, k-tiles, tail values per lane, waves per workgroup) of the matrix-core kernel the policy picks for the shape"""
    from vbmc_amd import _lib

    q = [ctypes.c_int() for _ in range(4)]
    kind = _lib.load().vbmc_entropy_plan(D, K, *[ctypes.byref(x) for x in q])
    if kind == 2:       # the lane kernel's class (K <= 16): with VBMC_ENT_KERNEL=mfma one k-tile on one wave
        return (D + 2 + 3) // 4, 1, 0, 1
    assert kind == 1
    return q[0].value, q[1].value, q[3].value, q[2].value


def test_the_matrix_runs_every_sample_layout_class():
    """every (QS, k-tiles, tail) class that takes the layout is run by some (D, K) of the matrix -- and so are shapes that do not"""
    want = {(qs, kt, tl) for qs in (1, 2, 3) for kt in (1, 2, 3) for tl in (0, 1, 2) if sl_class(qs, kt, tl)}
    ran = {plan_class(D, K)[:3] for D in SL_D for K in SL_K}
    assert {c for c in ran if sl_class(*c)} == want, sorted(want - ran)
    assert any(not sl_class(*c) for c in ran)


@pytest.mark.parametrize("K", SL_K)
@pytest.mark.parametrize("D", SL_D)
def test_sample_layout_against_the_oracle_on_the_device_stream(va, D, K, monkeypatch):
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")          # (small mixtures: not the lane kernel)
    p, gp, vp, theta = problem(100 + 13 * D + K, D, 30, K, 2)
    eng = va.default_engine()
    for Ns, seed in ((32, 11), (74, 12)):                   # Mh = 16: one full tile; Mh = 37: two full tiles and a partial one of 5
        eps = eng.ctx.rng_dump(D, K, 1, Ns, seed)[0]
        ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
        out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=seed)
        assert_matrix_core_one_wave(va, D, K)
        assert relerr(out["H"][0], ref["H"]) < RT_VAL
        blocks_ok(out["dH"][:, 0], ref["dH"], D, K)
        blocks_ok(out["dF"][:, 0], ref["dF"], D, K)


@pytest.mark.parametrize("K", [18, 50])
def test_sample_layout_against_the_valu_kernel(va, K, monkeypatch):
    """k_entropy (one lane per sample, no matrix cores, no shared code with the tile body) on the same device stream"""
    from vbmc_amd import _lib

    D, Ns, R_ = 10, 74, 3
    p, gp, vp, theta = problem(70 + K, D, 30, K, 2)
    thetas = theta[:, None] + 0.05 * np.random.default_rng(K).standard_normal((theta.size, R_))
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    m = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=21)
    assert_matrix_core_one_wave(va, D, K)
    monkeypatch.setenv("VBMC_ENT_KERNEL", "valu")
    v = va.negelcbo_batch(thetas, 0, vp, gp, Ns, True, 0, seed=21)
    assert va.default_engine().ctx.last_launch()[0] == _lib.ENTFORM_VALU
    assert relerr(m["H"], v["H"]) < 1e-13
    for r in range(R_):
        assert relerr(m["dH"][:, r], v["dH"][:, r]) < 1e-12


# ---------------------------------------------------------------- the siblings of the class, D = 10, K = 50
@pytest.fixture(scope="module")
def headline():
    return problem(61, 10, 80, 50, 20)


def test_sample_layout_in_the_launch_that_carries_the_log_joint_role(va, headline, monkeypatch):
    from vbmc_amd import _lib

    p, gp, vp, theta = headline
    monkeypatch.delenv("VBMC_ENT_CHUNKS", raising=False)
    monkeypatch.delenv("VBMC_LJ_CO", raising=False)
    Ns, seed = 3000, 5
    eps = va.default_engine().ctx.rng_dump(10, 50, 1, Ns, seed)[0]
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=seed)
    assert va.default_engine().ctx.last_launch() == (_lib.ENTFORM_MFMA, _lib.LJFORM_ROLE_MFMA)
    assert relerr(out["H"][0], ref["H"]) < RT_VAL and relerr(out["G"][0], ref["G"]) < RT_VAL
    blocks_ok(out["dH"][:, 0], ref["dH"], 10, 50)
    blocks_ok(out["dF"][:, 0], ref["dF"], 10, 50)


def test_sample_layout_in_parity_mode_block_sparse_mode_and_value_only(va, headline):
    """the headline shape's parity-mode kernel takes the layout; with a cutoff K = 50 is FOUR k-tiles (the block-sparse kernels have no
    component tail) and with that the column layout, like the value-only call: both are here to show that they are untouched.  The
    block-sparse kernels that do take the layout: test_sample_layout_in_block_sparse_mode."""
    p, gp, vp, theta = headline
    D, K, Ns = 10, 50, 74
    eps = np.random.default_rng(9).standard_normal((K, Ns // 2, D))
    ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
    d = va.negelcbo_batch(theta, 0, vp, gp, Ns, True, 0, eps=eps)                           # the caller's draws (the prefetching kernel)
    assert_matrix_core_one_wave(va, D, K)
    s_ = va.negelcbo_batch(theta, 0, vp, gp, Ns, True, 0, eps=eps, sparse_cutoff=100.0)    # block-sparse: four k-tiles, the column layout
    assert_matrix_core_one_wave(va, D, K)
    for out in (d, s_):
        assert relerr(out["H"][0], ref["H"]) < RT_VAL
        blocks_ok(out["dH"][:, 0], ref["dH"], D, K)
        blocks_ok(out["dF"][:, 0], ref["dF"], D, K)
    v = va.negelcbo_batch(theta, 0, vp, gp, Ns, False, 0, eps=eps)                          # value only: the column layout never existed there
    assert_matrix_core_one_wave(va, D, K)
    assert relerr(v["H"][0], ref["H"]) < RT_VAL and relerr(v["F"][0], ref["F"]) < RT_VAL


# block-sparse kernels have no component tail: k-tiles = ceil(K / 16).  Those that take the layout: three k-tiles at D = 7..10 (with the LDS
# re-read of u'), two and three at D = 3..6, one to three at D <= 2.
@pytest.mark.parametrize("D,K", [(10, 48), (9, 33), (7, 40), (6, 30), (5, 48), (2, 12), (2, 30), (1, 44)])
def test_sample_layout_in_block_sparse_mode(va, D, K, monkeypatch):
    """sparse_cutoff = 100 on a well separated mixture (k-tiles really are skipped) against the oracle, with the caller's draws and on the
    device stream (padded dimensions hold draws there), full and partial tiles"""
    monkeypatch.setenv("VBMC_ENT_KERNEL", "mfma")
    qs, kt = (D + 2 + 3) // 4, (K + 15) // 16
    assert sl_class(qs, kt, 0)
    p, gp, vp, theta = problem(200 + 13 * D + K, D, 30, K, 2)
    eng = va.default_engine()
    for Ns, seed in ((32, 31), (74, 32)):
        for eps, kw in ((np.random.default_rng(seed).standard_normal((K, Ns // 2, D)), None), (eng.ctx.rng_dump(D, K, 1, Ns, seed)[0], seed)):
            ref = R.negelcbo_vbmc(theta, 0, vp, gp, Ns, True, 0, eps=eps)
            if kw is None:
                out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, eps=eps[None], sparse_cutoff=100.0)
            else:
                out = va.negelcbo_batch(theta[:, None], 0, vp, gp, Ns, True, 0, seed=kw, sparse_cutoff=100.0)
            assert_matrix_core_one_wave(va, D, K)
            assert relerr(out["H"][0], ref["H"]) < RT_VAL
            blocks_ok(out["dH"][:, 0], ref["dH"], D, K)
            blocks_ok(out["dF"][:, 0], ref["dF"], D, K)

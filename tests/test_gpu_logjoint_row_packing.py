"""k_logjoint_mfma with the rows of the whole batch packed into its workgroups (vbmc_amd/csrc/elbo_kernels.h, elbo_pass.h): row
rho = r K + k, sixteen rows per wave, a workgroup = (hyper-sample, row group); the last chunk of the training set runs only the k-steps
that hold a point.  Shapes (D, K, N, S, R):
  (3, 5, 7, 2, 3)      15 rows of three restarts in ONE wave; N < 64: one chunk of two k-steps, the second with one point
  (10, 50, 70, 3, 5)   250 rows in four groups of 64: the groups straddle restart boundaries, the last is short (58 rows, its fourth wave
                       10); a full chunk and one of 6 points (two k-steps, the second half empty)
  (4, 16, 64, 2, 4)    exact fits: a wave per restart, one full chunk
  (2, 17, 1, 1, 1)     one restart (the launch as it was: two waves, the second with one row), one training point
Each: value and gradient against the oracle at the project's RT_VAL / RT_GRAD, restart by restart; against the VALU kernel k_logjoint at
1e-13 / 1e-12 (two device kernels, different order of summation); every restart of the batch BIT-identical to the same restart evaluated
alone (the order of points and chunks within a row does not depend on where the row sits); and the value-only form.

(The bound against the VALU kernel is what found the kernel's mis-typed constant sqrt(512 / ln 2) -- 2.7e-13 off, every exponent stretched
by 5.4e-13 of itself: at (4, 16, 64, 2, 4) G stood 1.29e-13 and dG 9.2e-13 from the VALU kernel and the oracle, with the constant right
1.2e-16 and 3.3e-15.)

The value-only form k_logjoint_mfma<DT, false> is the plan's choice only from S R >= 4 x 256 cells on (elbo_launch_plan.h), VBMC_LJ_KERNEL
or not: at the shapes' own R a value-only pass runs the VALU kernel, so the batch is repeated until it is that wide -- every copy of a
restart must then give the same bits, wherever its rows sit, and the value of the gradient form to 1e-13 (the value-only form adds each lane's
points first and the four point lanes last, the gradient form a k-step at a time: the same terms in another order)."""
import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests._cases import block_relerr, relerr
from tests.test_gpu_elbo import RT_GRAD, RT_VAL, problem

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 2, 3), (10, 50, 70, 3, 5), (4, 16, 64, 2, 4), (2, 17, 1, 1, 1)]
_cache = {}


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def case(shape):
    """the problem, the batch of thetas and the oracle's value and gradient per restart: computed once per shape"""
    if shape not in _cache:
        D, K, N, S, Rn = shape
        # (the generator takes the spread of y and of the best points for its scales: it needs a few points -- a training set of one is the
        # first of nine, under the hyper-parameters and the mixture made for the nine)
        p, gp, vp, theta = problem(700 + D + K, D, N if N >= 4 else 9, K, S)
        if N < 4:
            gp = R.gplite_post(p["hyp"], p["X"][:N], p["y"][:N], meanfun=p["meanfun"], noisefun=p["noisefun"], s2=p["s2"])
        Th = np.asfortranarray(theta[:, None] + 0.05 * np.random.default_rng(N).standard_normal((theta.size, Rn)))
        ref = [R.negelcbo_vbmc(Th[:, r], 0, vp, gp, 0, True, 0) for r in range(Rn)]
        _cache[shape] = (gp, vp, Th, ref)
    return _cache[shape]


def run(va, monkeypatch, kern, Th, vp, gp, grad=True):
    from vbmc_amd import _lib

    monkeypatch.setenv("VBMC_LJ_KERNEL", kern)
    out = va.negelcbo_batch(Th, 0, vp, gp, 0, grad, 0)
    return out, va.default_engine().ctx.last_launch()[1], _lib


@pytest.mark.parametrize("shape", SHAPES)
def test_packed_rows_against_the_oracle_and_the_valu_kernel(va, shape, monkeypatch):
    D, K, N, S, Rn = shape
    gp, vp, Th, ref = case(shape)
    m, form, _lib = run(va, monkeypatch, "mfma", Th, vp, gp)
    assert form == _lib.LJFORM_MFMA_GRAD, form
    v, form, _ = run(va, monkeypatch, "valu", Th, vp, gp)
    assert form in (_lib.LJFORM_VALU_SPLIT, _lib.LJFORM_VALU_WAVE), form
    for r in range(Rn):
        assert relerr(m["G"][r], ref[r]["G"]) < RT_VAL, (shape, r)
        err = block_relerr(m["dG"][:, r], ref[r]["dG"], D, K)
        assert max(err.values()) < RT_GRAD, (shape, r, err)
    eG = relerr(m["G"], v["G"])
    edG = max(relerr(m["dG"][:, r], v["dG"][:, r]) for r in range(Rn))
    print("shape %s: G %.2e dG %.2e against the VALU kernel" % (shape, eG, edG))
    assert eG < 1e-13
    assert edG < 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_every_restart_of_the_batch_has_the_bits_it_has_alone(va, shape, monkeypatch):
    D, K, N, S, Rn = shape
    gp, vp, Th, ref = case(shape)
    m, form, _lib = run(va, monkeypatch, "mfma", Th, vp, gp)
    assert form == _lib.LJFORM_MFMA_GRAD
    for r in range(Rn):
        one, form, _ = run(va, monkeypatch, "mfma", np.asfortranarray(Th[:, r:r + 1]), vp, gp)
        assert form == _lib.LJFORM_MFMA_GRAD
        assert np.array_equal(one["G"], m["G"][r:r + 1]) and np.array_equal(one["dG"][:, 0], m["dG"][:, r]), (shape, r)


@pytest.mark.parametrize("shape", SHAPES)
def test_value_only_form_equals_the_value_of_the_gradient_form(va, shape, monkeypatch):
    D, K, N, S, Rn = shape
    gp, vp, Th, ref = case(shape)
    reps = -(-1024 // (S * Rn))                      # copies of the batch until S R >= 4 x 256 cells (see above)
    Tw = np.asfortranarray(np.tile(Th, (1, reps)))
    g, form, _lib = run(va, monkeypatch, "mfma", Tw, vp, gp)
    assert form == _lib.LJFORM_MFMA_GRAD
    vo, form, _ = run(va, monkeypatch, "mfma", Tw, vp, gp, grad=False)
    assert form == _lib.LJFORM_MFMA_VALUE, form
    for r in range(Rn):
        assert relerr(vo["G"][r], ref[r]["G"]) < RT_VAL
        assert np.all(vo["G"][r::Rn] == vo["G"][r]) and np.all(g["G"][r::Rn] == g["G"][r]), (shape, r)     # every copy, wherever its rows sit
    e = relerr(vo["G"], g["G"])
    print("shape %s: value-only against the gradient form %.2e" % (shape, e))
    assert e < 1e-13
    g1, _, _ = run(va, monkeypatch, "mfma", Th, vp, gp)      # ... and the batch by itself
    assert np.array_equal(g1["G"], g["G"][:Rn])

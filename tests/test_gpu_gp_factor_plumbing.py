"""Host plumbing of the GP entry points (vbmc_amd/csrc/gp_factor.h, gp_pred.h): the three forms of gplite_nlZ's gradient leg, the optimistic
first try of the factorisation handing over to the checked noise-inflation loop, a vector that still fails after the loop, a posterior
whose hyper-samples take both branches adopted as a device handle, and the refusals of the two entry points that build a handle.

Expected values are the oracle's (oracle/vbmc_ref.py) at the tolerances tests/test_gpu_nlz.py and tests/test_gpu_gplite.py use for
the same quantities; the quadrature, which the oracle does not have, is held against tests/_quad_ref.py at tests/test_gpu_quad.py's."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _quad_ref as Q
from tests._cases import relerr
from tests.test_gpu_nlz import make_gp

pytestmark = pytest.mark.gpu

U8P = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def _nlz_vs_oracle(va, gp, H, grad=True):
    out = va.gplite_nlZ(H, gp) if grad else (va.gplite_nlZ(H, gp, nargout=1), None)
    for b in range(H.shape[1]):
        f, g = R.gplite_nlZ(H[:, b], gp)
        assert abs(out[0][b] - f) < 1e-10 * max(1.0, abs(f)), (b, out[0][b], f)          # test_nlz_batch_matches_oracle's
        if grad:
            assert relerr(out[1][:, b], g) < 1e-8, (b, relerr(out[1][:, b], g))
    return out


@pytest.mark.parametrize("N,B", [(48, 2), (528, 2), (528, 17)])
def test_nlz_gradient_forms(va, N, B):
    """D = 3.  N = 48, B = 2: the factor's inverse and alpha's backward solve in one launch (`combined`).  N = 528 (the first multiple
    of 16 above ASOLVE1_THREADS = 512), B = 2: alpha's solve on the second stream beside the inverse.  N = 528, B = 17: neither."""
    gp, draw = make_gp(np.random.default_rng(N + B), N, 3, 4, (1, 0, 0))
    H = np.stack([draw() for _ in range(B)], axis=1)
    _nlz_vs_oracle(va, gp, H)


def test_nlz_value_only(va):
    gp, draw = make_gp(np.random.default_rng(48), 48, 3, 4, (1, 0, 0))
    H = np.stack([draw() for _ in range(2)], axis=1)
    _nlz_vs_oracle(va, gp, H, grad=False)


# ---- one batch whose middle vector needs the noise-inflation loop -----------------------------------------------------------------
def _retry_batch():
    """Triplicated inputs, as test_cholesky_jitter_retry_matches_reference_semantics builds them (N = 48, D = 3).  The outer vectors
    carry sn = 0.05; the middle one sn2 = 1e-14 under sf2 = e^8: K + sn2 I is singular to rounding until the noise has been inflated."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((16, 3))
    X = np.vstack([X, X, X])
    y = rng.standard_normal(48)
    H = np.zeros((12, 3))
    H[3, :] = 4.0
    H[4, :] = [math.log(0.05), math.log(1e-7), math.log(0.05)]
    H[5, :] = 0.1
    gp = {"X": X, "y": y, "s2": None, "covfun": 1, "Ncov": 4, "noisefun": (1, 0, 0), "Nnoise": 1, "meanfun": 4, "Nmean": 7,
          "meanfun_extras": None, "intmeanfun": 0}
    return gp, H


@pytest.fixture(scope="module")
def retry_batch():
    gp, H = _retry_batch()
    ref = R.gplite_post(H, gp["X"], gp["y"], meanfun=4)
    mult = [p["sn2_mult"] for p in ref["post"]]
    assert mult[0] == 1.0 and mult[2] == 1.0 and mult[1] > 1.0        # on the CPU: exactly one vector retries
    return gp, H, ref


def _post_raw(va, gp, H, want_handle, need_L=True):
    """vbmc_gp_post itself, with or without gp_out; returns (alpha, L, sW, mult, lchol) and frees the handle."""
    from vbmc_amd._lib import f64, ptr
    from vbmc_amd.elbo import default_engine

    ctx = default_engine().ctx
    X, y, H = f64(gp["X"]), f64(gp["y"]), f64(H)
    N, D = X.shape
    Nhyp, S = H.shape
    alpha, sW = np.empty((N, S), order="F"), np.empty((N, S), order="F")
    L = np.empty((N, N, S), order="F") if need_L else None
    mult, lch = np.zeros(S), np.zeros(S, dtype=np.uint8)
    h = C.c_void_p()
    st = ctx.lib.vbmc_gp_post(ctx.h, N, D, S, Nhyp, 4, (C.c_int32 * 3)(1, 0, 0), ptr(X), ptr(y), None, ptr(H), ptr(alpha), ptr(L), ptr(sW),
                              ptr(mult), lch.ctypes.data_as(U8P), C.byref(h) if want_handle else None)
    if h:
        ctx.lib.vbmc_gp_free(ctx.h, h)
    return st, (alpha, L, sW, mult, lch)


def test_optimistic_try_fails_then_checked_loop_nlz(va, retry_batch):
    gp, H, ref = retry_batch
    f, g = va.gplite_nlZ(H, gp)
    # the middle vector: how many x10 steps it takes is decided by rounding in the factorisation, and the accepted matrix has condition
    # ~1e16 / mult (test_nlz_low_noise_branch_and_retries): finite is what can be asked of it
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    for b in (0, 2):                                                  # the neighbours: the bits of the same vector run alone
        f1, g1 = va.gplite_nlZ(H[:, b], gp)
        assert f[b] == f1 and np.array_equal(g[:, b], g1), b
        fr, gr = R.gplite_nlZ(H[:, b], gp)
        assert abs(f[b] - fr) < 1e-10 * max(1.0, abs(fr)) and relerr(g[:, b], gr) < 1e-8


@pytest.mark.parametrize("want_handle", [True, False])
def test_optimistic_try_fails_then_checked_loop_post(va, retry_batch, want_handle):
    gp, H, ref = retry_batch
    st, (alpha, L, sW, mult, lch) = _post_raw(va, gp, H, want_handle)
    assert st == 0
    assert list(lch) == [1, 0, 1] and mult[0] == 1.0 and mult[2] == 1.0 and mult[1] > 1.0
    assert np.all(np.isfinite(alpha)) and np.all(np.isfinite(L))
    for s in (0, 2):
        st1, (a1, L1, w1, m1, l1) = _post_raw(va, gp, H[:, s:s + 1], want_handle)
        assert st1 == 0
        assert np.array_equal(alpha[:, s], a1[:, 0]) and np.array_equal(L[:, :, s], L1[:, :, 0]) and np.array_equal(sW[:, s], w1[:, 0]), s
        b = ref["post"][s]
        assert relerr(L[:, :, s], b["L"]) < 1e-9 and relerr(alpha[:, s], b["alpha"]) < 1e-7      # test_gp_post_matches_oracle's


# ---- a vector that still fails after ten inflations ------------------------------------------------------------------------------------
def test_vector_failing_after_ten_inflations(va):
    """sf2 = exp(800) overflows: the kernel matrix is not finite whatever the noise multiplier.  vbmc_gp_nlz: NaN for that row only;
    vbmc_gp_post: VBMC_ERR_NOT_POSDEF."""
    from vbmc_amd._lib import VBMC_ERR_NOT_POSDEF

    gp, draw = make_gp(np.random.default_rng(7), 48, 3, 4, (1, 0, 0))
    H = np.stack([draw() for _ in range(3)], axis=1)
    H[3, 1] = 400.0
    f, g = va.gplite_nlZ(H, gp)
    assert np.isnan(f[1]) and np.all(np.isnan(g[:, 1]))
    for b in (0, 2):
        fr, gr = R.gplite_nlZ(H[:, b], gp)
        assert abs(f[b] - fr) < 1e-10 * max(1.0, abs(fr)) and relerr(g[:, b], gr) < 1e-8
    v = va.gplite_nlZ(H, gp, nargout=1)
    assert np.isnan(v[1])
    for b in (0, 2):
        fr = R.gplite_nlZ(H[:, b], gp)[0]
        assert abs(v[b] - fr) < 1e-10 * max(1.0, abs(fr))
    for want_handle in (True, False):
        st, _ = _post_raw(va, gp, H, want_handle)
        assert st == VBMC_ERR_NOT_POSDEF
    st, _ = _post_raw(va, gp, H[:, [0, 2]], True)                      # the context goes on working
    assert st == 0


# ---- a posterior of both branches, adopted ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_L", [True, False])
def test_mixed_branch_posterior_adopted(va, need_L):
    """S = 3, Lchol = [1, 0, 1] (the middle sample's minimum noise 9e-8 < 1e-6), N = 48: with L asked for and with the handle only;
    then gplite_pred and gplite_quad on 20 points, per hyper-sample and averaged, through the adopted handle."""
    D, N, S = 3, 48, 3
    ref, p = Q.mixed_gp(31, D, N, S, 4)
    hyp = np.stack([q["hyp"] for q in ref["post"]], axis=1)
    gp = va.gplite_post(hyp, p["X"], p["y"], 1, 4, need_L=need_L)
    assert [q["Lchol"] for q in gp["post"]] == [True, False, True] == [q["Lchol"] for q in ref["post"]]
    for a, b in zip(gp["post"], ref["post"]):
        assert a["sn2_mult"] == b["sn2_mult"] == 1.0 and relerr(a["sW"], b["sW"]) < 1e-14
        tolL, tolA = (1e-9, 1e-7) if b["Lchol"] else (1e-6, 1e-6)      # test_gp_post_matches_oracle's, test_low_noise_branch's
        assert relerr(a["alpha"], b["alpha"]) < tolA
        assert (a["L"] is None) if not need_L else relerr(a["L"], b["L"]) < tolL
    rng = np.random.default_rng(5)
    Xs = 1.3 * rng.standard_normal((20, D))
    sg = np.array([0.3, 0.0, 0.2])
    nfkk = Q.nf_kk(ref, sg)
    for ss in (True, False):
        o = va.gplite_pred(gp, Xs, None, None, ss)
        r = R.gplite_pred(ref, Xs, None, None, ssflag=ss)
        for x, z in zip(o, r):
            assert np.asarray(x).shape == np.asarray(z).shape
        assert relerr(o[0], r[0]) < 1e-6 and relerr(o[2], r[2]) < 1e-6                                    # test_low_noise_branch's
        assert np.max(np.abs(o[1] - r[1])) < 1e-6 and np.max(np.abs(o[3] - r[3])) < 1e-6
        F, V = va.gplite_quad(gp, Xs, sg, ss)
        Fr, Vr = Q.gplite_quad(ref, Xs, sg[None, :], ss)
        assert np.asarray(F).shape == np.asarray(Fr).shape
        assert relerr(F, Fr) < 1e-9 and np.max(np.abs(V - Vr)) < 1e-9 * np.max(nfkk)                      # test_gpu_quad._check's


# ---- the refusals of the entry points that build a handle ------------------------------------------------------------------------------
def test_refused_handles_stay_null_and_the_context_goes_on(va):
    from vbmc_amd import elbo as E
    from vbmc_amd._lib import VBMC_ERR_INVALID, VBMC_ERR_UNSUPPORTED, f64, ptr
    from vbmc_amd.gplite import _device_gp_with_noise

    D, N, S = 3, 48, 3
    ref, p = Q.mixed_gp(31, D, N, S, 4)
    hyp = np.stack([q["hyp"] for q in ref["post"]], axis=1)
    eng = E.Engine(0)
    gp = va.gplite_post(hyp, p["X"], p["y"], 1, 4, engine=eng)
    dgp = _device_gp_with_noise(eng, gp)
    ctx, lib = eng.ctx, eng.ctx.lib
    rng = np.random.default_rng(3)

    def create(Na, per_s, fs2a):
        xa = f64(rng.standard_normal((Na, D * (S if per_s else 1))))
        h = C.c_void_p()
        st = lib.vbmc_acq_is_create(ctx.h, dgp.h, Na, ptr(xa), per_s, None, ptr(fs2a), None, C.byref(h))
        return st, h

    st, h = create(256 + 1, 0, None)                                   # VBMC_LIM_NA = 256 (vbmc_get_limits)
    assert st == VBMC_ERR_UNSUPPORTED and not h
    assert "importance points not accelerated" in lib.vbmc_last_error(ctx.h).decode()
    st, h = create(32, 1, None)
    assert st == VBMC_ERR_INVALID and not h
    assert "need fs2a from the caller" in lib.vbmc_last_error(ctx.h).decode()
    st, h = create(32, 0, None)                                        # a valid call on the same context
    assert st == 0 and h
    lib.vbmc_acq_is_free(ctx.h, h)

    xstar = 0.5 * rng.standard_normal((1, D))
    Xn = f64(np.vstack([gp["X"], xstar]))
    sn2_eff = f64(np.array([math.exp(2.0 * q["hyp"][D + 1]) * q["sn2_mult"] for q in gp["post"]]))
    one = f64(np.ones(S))
    for mstar, vstar in ((one, None), (None, one)):
        h = C.c_void_p()
        st = lib.vbmc_gp_rank1_update(ctx.h, dgp.h, ptr(Xn), C.c_double(0.3), ptr(mstar), ptr(vstar), ptr(sn2_eff), None, None, C.byref(h))
        assert st == VBMC_ERR_INVALID and not h
        assert "mstar and vstar go together" in lib.vbmc_last_error(ctx.h).decode()
    g1 = va.gplite_post_rank1(gp, xstar, 0.3, engine=eng)             # a valid append on the same context, against the oracle's
    r1 = R.gplite_post_rank1(ref, xstar.reshape(-1), 0.3)
    for a, c in zip(g1["post"], r1["post"]):
        assert relerr(a["alpha"], c["alpha"]) < (1e-7 if c["Lchol"] else 1e-5)       # test_rank1_update_equals_full_posterior's, ..._low_noise_branch's

"""GPU: the MEX gateway's 'gp_quad' and 'acq_delta' commands, executed through the mock of the mx* API (tests/mock_mex/), return bit for
bit what the ctypes mirror returns for the same call -- both sit on vbmc_gp_quad / vbmc_acq_eval_delta and the calls are deterministic."""
import numpy as np
import pytest

from tests import _quad_ref as Q
from tests._mex import MexError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def _gp_struct(gp):
    post = [{"hyp": p["hyp"].reshape(-1, 1), "alpha": p["alpha"].reshape(-1, 1), "sW": p["sW"].reshape(-1, 1), "L": np.asfortranarray(p["L"]),
             "sn2_mult": float(p["sn2_mult"]), "Lchol": bool(p["Lchol"])} for p in gp["post"]]
    return {"X": np.asfortranarray(gp["X"]), "y": gp["y"].reshape(-1, 1), "meanfun": float(gp["meanfun"]), "covfun": 1.0,
            "noisefun": np.array(gp["noisefun"], dtype=np.float64).reshape(1, -1), "Ncov": float(gp["Ncov"]), "Nnoise": float(gp["Nnoise"]),
            "Nmean": float(gp["Nmean"]), "post": post}


def _setup():
    from tests.test_gpu_quad import _acq_setup

    gp, vp, Xs, st, rng = _acq_setup(7, 4, 60, 5, 3)
    return gp, vp, np.asfortranarray(Xs[:90]), st


def test_gp_quad_command_equals_the_ctypes_call(mex):
    import vbmc_amd as va

    gp, vp, mu, st = _setup()
    sg = vp["delta"].reshape(1, -1)
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    try:
        for ss in (1, 0):
            F, V = va.gplite_quad(gp, mu, sg, bool(ss))
            f, v = mex.call(2, "gp_quad", h, mu, sg, float(ss), 3.0)
            assert f.shape == ((90, 3) if ss else (90, 1))
            assert np.array_equal(f.reshape(F.shape), F) and np.array_equal(v.reshape(V.shape), V)
        (f1,) = mex.call(1, "gp_quad", h, mu, np.repeat(sg, 90, axis=0), 1.0, 3.0)        # equal rows; one output
        assert np.array_equal(f1, va.gplite_quad(gp, mu, sg, True, nargout=1))
        with pytest.raises(MexError) as e:                                                # a sigma row per point
            mex.call(1, "gp_quad", h, mu, np.abs(mu) + 0.1, 1.0, 3.0)
        assert e.value.identifier == "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:
            mex.call(1, "gp_quad", h, mu, sg[:, :3], 1.0, 3.0)
        assert e.value.identifier == "vbmc_hip:usage"
    finally:
        mex.call(0, "gp_free", h)


def test_acq_delta_command_equals_the_ctypes_call(mex):
    import vbmc_amd as va

    gp, vp, Xs, st = _setup()
    vps = {"K": float(vp["K"]), "mu": np.asfortranarray(vp["mu"]), "sigma": vp["sigma"].reshape(1, -1), "lambda": vp["lambda"].reshape(-1, 1),
           "w": vp["w"].reshape(1, -1)}
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    try:
        for aid, name in enumerate(("acqf_vbmc", "acqflog_vbmc", "acqus_vbmc")):
            acq, fbar, vtot = va.acqwrapper_vbmc(Xs, vp, gp, st, False, name, None, nargout=3, delta_quad=True)
            a, fb, vt = mex.call(3, "acq_delta", h, Xs, float(aid), vps, st["ymax"], 1.0, st["TolGPVar"], vp["delta"].reshape(1, -1))
            assert np.array_equal(a[:, 0], acq) and np.array_equal(fb[:, 0], fbar) and np.array_equal(vt[:, 0], vtot)
        (a1,) = mex.call(1, "acq_delta", h, Xs, 0.0, vps, st["ymax"], 1.0, st["TolGPVar"], vp["delta"].reshape(1, -1))
        assert np.array_equal(a1[:, 0], va.acqwrapper_vbmc(Xs, vp, gp, st, False, "acqf_vbmc", None, delta_quad=True))
        with pytest.raises(MexError):                                                     # all-zero delta: the caller wants 'acq'
            mex.call(1, "acq_delta", h, Xs, 0.0, vps, st["ymax"], 1.0, st["TolGPVar"], np.zeros((1, 4)))
        with pytest.raises(MexError) as e:                                                # the IQR ids stay refused
            mex.call(1, "acq_delta", h, Xs, 10.0, vps, st["ymax"], 1.0, st["TolGPVar"], vp["delta"].reshape(1, -1))
        assert e.value.identifier == "vbmc_hip:unsupported"
    finally:
        mex.call(0, "gp_free", h)

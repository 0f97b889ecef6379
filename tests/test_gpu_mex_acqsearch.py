"""GPU: the MEX gateway's 'acq_search' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror returns for the same call -- both sit on vbmc_acq_search and the call is deterministic given the seed or the normals."""
import numpy as np
import pytest

from tests import _acqsearch_ref as A
from tests._mex import MexError
from tests.test_gpu_mex_quad import _gp_struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def _vp_struct(vp):
    return {"K": float(vp["K"]), "mu": np.asfortranarray(vp["mu"]), "sigma": vp["sigma"].reshape(1, -1), "lambda": vp["lambda"].reshape(-1, 1),
            "w": vp["w"].reshape(1, -1)}


@pytest.mark.parametrize("name", ["D3", "sn2"])
def test_acq_search_command_equals_the_ctypes_call(mex, name):
    import vbmc_amd as va

    c = A.build_case(name)
    gp, vp, st = c["gp"], c["vp"], c["st"]
    aid = {"acqf": 0, "acqflog": 1, "acqus": 2, "acqfsn2": 3}[c["acq"]]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)  # noqa: E731
    base = [float(aid), _vp_struct(vp), st["ymax"], float(st["VarianceRegularizedAcqFcn"]), st["TolGPVar"], col(c["x0"]), col(c["insigma"]),
            col(c["LB"]), col(c["UB"])]
    extra = [st["gplengthscale"].reshape(1, -1), np.asfortranarray(gp["X_rescaled"]), col(gp["sn2new"])] if aid == 3 else []
    tol = dict(TolX=1e-11 * float(np.max(c["insigma"])), TolFun=1e-12, TolHistFun=1e-13)
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    try:
        for kw, opts in ((dict(seed=77, MaxFunEvals=140), {"Seed": 77.0, "MaxFunEvals": 140.0}),
                         (dict(Z=c["Z"], MaxIter=15), {"Z": np.asfortranarray(c["Z"]), "MaxIter": 15.0})):
            r = va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], vp, gp, st, c["acq"] + "_vbmc", **tol, **kw)
            xmin, fmin, out = mex.call(3, "acq_search", h, *base, dict({k: float(v) for k, v in tol.items()}, **opts), *extra)
            assert np.array_equal(xmin[:, 0], r["xmin"]) and fmin[0, 0] == r["fmin"]
            assert np.array_equal(out["xbest"][:, 0], r["xbest"]) and out["fbest"][0, 0] == r["fbest"]
            assert np.array_equal(out["xmean"][:, 0], r["xmean"]) and out["sigma"][0, 0] == r["sigma"] and np.array_equal(out["C"], r["C"])
            assert (out["evals"][0, 0], out["generations"][0, 0]) == (r["evals"], r["generations"])
            assert va.acq.SEARCH_STOP[int(out["stop"][0, 0])] == r["stop"]
        (x1,) = mex.call(1, "acq_search", h, *base, {"Seed": 77.0, "MaxFunEvals": 140.0, **{k: float(v) for k, v in tol.items()}}, *extra)
        assert x1.shape == (c["D"], 1)
        with pytest.raises(MexError) as e:                                                 # the IQR ids are refused
            mex.call(1, "acq_search", h, 10.0, *base[1:], {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:                                                 # vp.delta > 0
            mex.call(1, "acq_search", h, base[0], dict(base[1], delta=np.full((1, c["D"]), 0.1)), *base[2:], {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:                                                 # a box of the wrong length
            mex.call(1, "acq_search", h, *base[:8], col(c["UB"])[:-1], {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:usage"
        (x2,) = mex.call(1, "acq_search", h, *base, {"MaxIter": 3.0}, *extra)                # the context is still usable
        assert np.all(x2[:, 0] >= c["LB"]) and np.all(x2[:, 0] <= c["UB"])
    finally:
        mex.call(0, "gp_free", h)

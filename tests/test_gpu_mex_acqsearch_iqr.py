"""GPU: the MEX gateway's 'acq_search_iqr' command after 'is_create', executed through the mock of the mx* API (tests/mock_mex/), returns
bit for bit what the ctypes mirror returns for the same call -- both sit on vbmc_acq_is_create and vbmc_acq_search_iqr and the call is
deterministic given the seed or the normals."""
import numpy as np
import pytest

from tests import _acqsearch_iqr_ref as I
from tests._mex import MexError
from tests.test_gpu_mex_acqsearch import _vp_struct
from tests.test_gpu_mex_quad import _gp_struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def test_acq_search_iqr_command_equals_the_ctypes_call(mex):
    import vbmc_amd as va

    c = I.build_case("D3")
    gp, vp, st = c["gp"], c["vp"], c["st"]
    ais = st["ActiveImportanceSampling"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)  # noqa: E731
    base = [10.0, _vp_struct(vp), float(st["VarianceRegularizedAcqFcn"]), st["TolGPVar"], col(c["x0"]), col(c["insigma"]), col(c["LB"]), col(c["UB"])]
    extra = [st["gplengthscale"].reshape(1, -1), np.asfortranarray(gp["X_rescaled"]), col(gp["sn2new"])]
    tol = dict(TolX=1e-11 * float(np.max(c["insigma"])), TolFun=1e-12, TolHistFun=1e-13)
    ftol = {k: float(v) for k, v in tol.items()}
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    hh = np.uint64(h[0, 0])
    his = mex.call(1, "is_create", hh, np.asfortranarray(ais["Xa"]), None, None, None)[0]
    hi = np.uint64(his[0, 0])
    st_dev = dict(st, ActiveImportanceSampling={"Xa": ais["Xa"]})            # the same state: computed on the device from Xa
    try:
        for kw, opts in ((dict(seed=77, MaxFunEvals=140), {"Seed": 77.0, "MaxFunEvals": 140.0}),
                         (dict(Z=c["Z"], MaxIter=10), {"Z": np.asfortranarray(c["Z"]), "MaxIter": 10.0})):
            r = va.acq_search(c["x0"], c["insigma"], c["LB"], c["UB"], vp, gp, st_dev, "acqviqr_vbmc", **tol, **kw)
            xmin, fmin, out = mex.call(3, "acq_search_iqr", hh, hi, *base, dict(ftol, **opts), *extra)
            assert np.array_equal(xmin[:, 0], r["xmin"]) and fmin[0, 0] == r["fmin"]
            assert np.array_equal(out["xbest"][:, 0], r["xbest"]) and out["fbest"][0, 0] == r["fbest"]
            assert np.array_equal(out["xmean"][:, 0], r["xmean"]) and out["sigma"][0, 0] == r["sigma"] and np.array_equal(out["C"], r["C"])
            assert (out["evals"][0, 0], out["generations"][0, 0]) == (r["evals"], r["generations"])
            assert va.acq.SEARCH_STOP[int(out["stop"][0, 0])] == r["stop"]
        with pytest.raises(MexError) as e:                                                 # an id that is no IQR function
            mex.call(1, "acq_search_iqr", hh, hi, 3.0, *base[1:], {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:                                                 # the three noise inputs are not optional here
            mex.call(1, "acq_search_iqr", hh, hi, *base, {"MaxIter": 3.0})
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                                 # the state handle lost its class
            mex.call(1, "acq_search_iqr", hh, float(hi), *base, {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                                 # a box of the wrong length
            mex.call(1, "acq_search_iqr", hh, hi, *base[:7], col(c["UB"])[:-1], {"MaxIter": 3.0}, *extra)
        assert e.value.identifier == "vbmc_hip:usage"
        (x2,) = mex.call(1, "acq_search_iqr", hh, hi, *base, {"MaxIter": 3.0}, *extra)     # the session goes on
        assert np.all(x2[:, 0] >= c["LB"]) and np.all(x2[:, 0] <= c["UB"])
    finally:
        mex.call(0, "is_free", hi)
        mex.call(0, "gp_free", hh)

"""GPU: the MEX gateway's 'acq_is_sample' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what
the ctypes mirror returns for the same call (case B of tests/_issample_ref.py) -- both sit on vbmc_acq_is_sample and the call is
deterministic given the seed or the uniforms -- and its state handle is one 'acq_iqr' accepts."""
import numpy as np
import pytest

from tests import _issample_ref as I
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


def test_acq_is_sample_command_equals_the_ctypes_call(mex):
    from vbmc_amd.acq import importance_sample_device

    c = I.build_case("B")
    gp = c["gp"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)  # noqa: E731
    x0 = np.asfortranarray(np.transpose(c["x0"], (1, 2, 0)))                          # W x D x S
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    hh = np.uint64(h[0, 0])
    handles = []
    try:
        for kw, opts in ((dict(seed=77, spec=3), {"Seed": 77.0, "Spec": 3.0, "Thin": float(c["thin"])}),
                         (dict(uniforms=c["U"], spec=2), {"U": np.asfortranarray(c["U"]), "Spec": 2.0, "Thin": float(c["thin"])})):
            r = importance_sample_device(gp, c["x0"], c["LB"], c["UB"], c["Nm"], thin=c["thin"], want_state=False, **kw)
            Xa, lnw, fs2a, his, out = mex.call(5, "acq_is_sample", hh, x0, col(c["LB"]), col(c["UB"]), float(c["Nm"]), opts)
            handles.append(np.uint64(his[0, 0]))
            assert np.array_equal(Xa, r["Xa"]) and np.array_equal(lnw, r["lnw"]) and np.array_equal(fs2a, r["fs2a"])
            assert np.array_equal(out["logp"], r["logp"])
            assert (out["funccount"][0, 0], out["performed"][0, 0], out["rounds"][0, 0]) == (r["funccount"], r["performed"], r["rounds"])
        with pytest.raises(MexError) as e:                                             # an odd number of walkers
            mex.call(1, "acq_is_sample", hh, np.asfortranarray(x0[:5]), col(c["LB"]), col(c["UB"]), float(c["Nm"]), {"Seed": 1.0})
        assert e.value.identifier != "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:                                             # a box of the wrong length
            mex.call(1, "acq_is_sample", hh, x0, col(c["LB"])[:-1], col(c["UB"]), float(c["Nm"]), {"Seed": 1.0})
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                             # opts is not a struct
            mex.call(1, "acq_is_sample", hh, x0, col(c["LB"]), col(c["UB"]), float(c["Nm"]), 3.0)
        assert e.value.identifier == "vbmc_hip:usage"
        (X2,) = mex.call(1, "acq_is_sample", hh, x0, col(c["LB"]), col(c["UB"]), 4.0, {"Seed": 2.0})      # the session goes on
        assert X2.shape == (4, c["D"], c["S"])
    finally:
        for hi in handles:
            mex.call(0, "is_free", hi)
        mex.call(0, "gp_free", hh)

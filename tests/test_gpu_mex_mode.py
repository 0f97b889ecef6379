"""GPU: the MEX gateway's 'vp_mode' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror (vbmc_amd.vptools.vbmc_mode) returns for the same call -- x, and with more outputs fval and the winning start; what
the shim stores as vp.mode is that x (vbmc_mode(..., nargout=2) stores the same) --, and an unsupported request comes back as
'vbmc_hip:unsupported', on which the shim falls through."""
import numpy as np
import pytest

from tests import _mode_ref as M
from tests._mex import MexError
from tests.test_gpu_mex_vptools import mx_vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def test_vp_mode_equals_the_ctypes_call(mex):
    from vbmc_amd import vptools as V

    for name in ("d4k65_all", "d25k130_mix", "d1k1"):
        vp, nmax = M.make_case(name)
        s, D = mx_vp(vp), vp["D"]
        for origflag in (1.0, 0.0):
            rx, det = V.vbmc_mode(vp, nmax, bool(origflag), details=True)
            x, fval, idx = mex.call(3, "vp_mode", s, float(nmax), origflag, 1e-6)
            assert x.shape == (1, D) and np.array_equal(x.reshape(-1), rx), (name, origflag)
            assert fval.reshape(-1)[0] == det["fval"] and int(idx.reshape(-1)[0]) == det["idx"]
            (x1,) = mex.call(1, "vp_mode", s, float(nmax), origflag, 1e-6)
            assert np.array_equal(x1, x)
            _, vp2 = V.vbmc_mode(vp, nmax, bool(origflag), nargout=2)
            assert (np.array_equal(vp2["mode"], x.reshape(-1))) if origflag else ("mode" not in vp2)      # what the shim stores
    vp, nmax = M.make_case("d4k65_all")
    (x0,) = mex.call(1, "vp_mode", mx_vp(vp), 0.0, 1.0, 1e-6)                           # nmax <= 0: the library's 20
    assert np.array_equal(x0.reshape(-1), V.vbmc_mode(vp, 20, True))
    bad = dict(vp, trinfo=dict(vp["trinfo"], type=np.array([0, 9, 2, 3])))
    with pytest.raises(MexError) as e:
        mex.call(1, "vp_mode", mx_vp(bad), 20.0, 1.0, 1e-6)
    assert e.value.identifier == "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:                                                 # tol_grad = 0: an error, not a fall-through
        mex.call(1, "vp_mode", mx_vp(vp), 20.0, 1.0, 0.0)
    assert e.value.identifier != "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:                                                 # too few arguments: refused before a device call
        mex.call(1, "vp_mode", mx_vp(vp), 20.0, 1.0)
    assert e.value.identifier == "vbmc_hip:usage"
    (again,) = mex.call(1, "vp_mode", mx_vp(vp), float(nmax), 1.0, 1e-6)               # the session goes on
    assert np.array_equal(again.reshape(-1), V.vbmc_mode(vp, nmax, True))

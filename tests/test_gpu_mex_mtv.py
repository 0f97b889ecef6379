"""GPU: the MEX gateway's 'vp_mtv' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror (vbmc_amd.vptools.vbmc_mtv) returns for the same call, in every output and for every number of outputs, and an
unsupported request comes back as 'vbmc_hip:unsupported', on which the shim falls through.  (The command runs the reference's mesh
and quadrature sizes, 2^13 and 1e5; Ns is kept small.)"""
import numpy as np
import pytest

from tests import _mtv_ref as M
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


def test_vp_mtv_equals_the_ctypes_call(mex):
    from vbmc_amd import vptools as V

    for name in ("bounds", "empty"):
        vp1, vp2 = M.make_pair(name)[:2]
        s1, s2, D = mx_vp(vp1), mx_vp(vp2), vp1["D"]
        rm, r1, r2 = V.vbmc_mtv(vp1, vp2, 1003, seed=4, nargout=3)
        mtv, x1, x2 = mex.call(3, "vp_mtv", s1, s2, 1003.0, 4.0)
        assert mtv.shape == (1, D) and np.array_equal(mtv.reshape(-1), rm) and np.array_equal(x1, r1) and np.array_equal(x2, r2)
        mtv2, y1 = mex.call(2, "vp_mtv", s1, s2, 1003.0, 4.0)
        (mtv1,) = mex.call(1, "vp_mtv", s1, s2, 1003.0, 4.0)
        assert np.array_equal(mtv2, mtv) and np.array_equal(y1, r1) and np.array_equal(mtv1, mtv)
    g0, g1 = mx_vp(M._gauss(1, 0.0, 1.0)), mx_vp(M._gauss(1, 0.5, 1.0))
    with pytest.raises(MexError) as e:                                                 # the fminbnd branch
        mex.call(1, "vp_mtv", g0, g1, 5.0, 4.0)
    assert e.value.identifier == "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:                                                 # vp2 is a sample matrix: the shim never sends it
        mex.call(1, "vp_mtv", g0, np.zeros((10, 1)), 100.0, 4.0)
    assert e.value.identifier == "vbmc_hip:usage"
    (again,) = mex.call(1, "vp_mtv", g0, g1, 1003.0, 4.0)                              # the session goes on
    assert np.array_equal(again.reshape(-1), V.vbmc_mtv(M._gauss(1, 0.0, 1.0), M._gauss(1, 0.5, 1.0), 1003, seed=4))

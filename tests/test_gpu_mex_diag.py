"""GPU: the MEX gateway's 'vp_diag' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror (vbmc_amd.vptools.vp_diagnostics) returns for the same call, in every output and for one to four outputs, and an
unsupported request comes back as 'vbmc_hip:unsupported', on which the shim falls through.  (The command runs the reference's mesh
and quadrature sizes, 2^13 and 1e5; Ns is kept small.)"""
import numpy as np
import pytest

from tests import _diag_ref as R
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


def test_vp_diag_equals_the_ctypes_call(mex):
    from vbmc_amd import vptools as V

    for vps in (R.runs("B", 3), [M._gauss(1, 0.0, 1.0), M._gauss(1, 0.5, 1.3)]):
        n, D = len(vps), vps[0]["D"]
        ref = V.vp_diagnostics(vps, 1003, seed=4, draws=True)
        s = [mx_vp(v) for v in vps]
        kl, mm, mtv, xx = mex.call(4, "vp_diag", 1003.0, 4.0, *s)
        assert kl.shape == (n, n) and mm.shape == (n, n) and mtv.shape == (D, n, n) and xx.shape == (1003, D, n)
        assert np.array_equal(kl, ref["kl_mat"]) and np.array_equal(mm, ref["maxmtv_mat"])
        assert np.array_equal(mtv.transpose(2, 1, 0), ref["mtv"])                      # D x R x R, symmetric in the runs
        assert np.array_equal(xx.transpose(2, 0, 1), ref["xx"])
        for nout in (3, 2, 1):
            got = mex.call(nout, "vp_diag", 1003.0, 4.0, *s)
            assert len(got) == nout
            for a, b in zip(got, (kl, mm, mtv)):
                assert np.array_equal(a, b), nout
    g = [mx_vp(M._gauss(1, 0.1 * i, 1.0)) for i in range(33)]
    with pytest.raises(MexError) as e:                                                 # the fminbnd branch
        mex.call(1, "vp_diag", 5.0, 4.0, g[0], g[1])
    assert e.value.identifier == "vbmc_hip:unsupported" and "run 1, dimension 1" in e.value.message
    with pytest.raises(MexError) as e:                                                 # more runs than a call takes
        mex.call(1, "vp_diag", 63.0, 4.0, *g)
    assert e.value.identifier == "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:                                                 # no run at all
        mex.call(1, "vp_diag", 100.0, 4.0)
    assert e.value.identifier == "vbmc_hip:usage"
    with pytest.raises(MexError) as e:                                                 # a sample matrix is not a posterior
        mex.call(1, "vp_diag", 100.0, 4.0, g[0], np.zeros((10, 1)))
    assert e.value.identifier == "vbmc_hip:usage"
    (again,) = mex.call(1, "vp_diag", 1003.0, 4.0, g[0], g[5])                         # the session goes on
    assert np.array_equal(again, V.vp_diagnostics([M._gauss(1, 0.0, 1.0), M._gauss(1, 0.5, 1.0)], 1003, seed=4)["kl_mat"])

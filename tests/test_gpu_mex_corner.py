"""GPU: the MEX gateway's 'vp_corner' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror (vbmc_amd.vptools.vbmc_plot_data / cornerplot_data) returns for the same call, in every output and for every number of
outputs, for a posterior and for a sample matrix; an unsupported request comes back as 'vbmc_hip:unsupported', on which the shim
reports ok = false."""
import numpy as np
import pytest

from tests import _corner_ref as R
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


def same(out, ref, n):
    """the first n outputs of the command against the ctypes dict (the library's column-major res x res x P is the dict's [pp][row][column] transposed)"""
    xx, b, h, q, de, bw, ts, c2 = (list(out) + [None] * 8)[:8]
    D = ref["xx"].shape[1]
    assert xx.shape == ref["xx"].shape and np.array_equal(xx, ref["xx"])
    if n > 1:
        assert b.shape == (2, D) and np.array_equal(b.T, ref["bounds"])
    if n > 2:
        assert h.dtype == np.float64 and np.array_equal(h.T, ref["hist"])
    if n > 3:
        assert q.shape == (len(ref["p"]), D) and np.array_equal(q.T, ref["quant"])
    P = len(ref["pairs"])
    if n > 4:
        assert de.shape == ((ref["res"], ref["res"], P) if P != 1 else (ref["res"], ref["res"]))      # (a trailing singleton is dropped, as MATLAB does)
        de = de.reshape(ref["res"], ref["res"], P)
        for pp in range(P):
            assert np.array_equal(de[:, :, pp], ref["density"][pp], equal_nan=True), pp
    if n > 5:
        assert np.array_equal(bw.T, ref["bandwidth"], equal_nan=True)
    if n > 6:
        assert np.array_equal(ts.reshape(-1), ref["tstar"], equal_nan=True)
    if n > 7:
        c2 = c2.reshape(ref["res"], ref["res"], P)
        for pp in range(P):
            assert np.array_equal(c2[:, :, pp], ref["counts2"][pp]), pp


def test_vp_corner_equals_the_ctypes_call(mex):
    from vbmc_amd import vptools as V

    for name in ("three32", "cut1", "one"):
        vp, Ns, res, bounds, bal = R.make_case(name)
        b = R.cut_bounds(V.vbmc_rnd(vp, Ns, True, bool(bal), seed=4, nargout=1)) if isinstance(bounds, str) else None
        ref = V.vbmc_plot_data(vp, Ns, seed=4, balanceflag=bal, bounds=b, res=res, p=(0.5, 0.1), stages=True)
        args = (mx_vp(vp), None, float(Ns), 4.0, float(bal), None if b is None else np.asfortranarray(b.T), float(res), 0.0, np.array([[0.5, 0.1]]))
        for n in (8, 5, 1):
            same(mex.call(n, "vp_corner", *args), ref, n)
    X, b = R.edge_matrix()
    ref = V.cornerplot_data(X, b, res=0, nbins=0, p=(0.5,), stages=True)                         # the shim's call: the library's 64 and 40
    assert ref["res"] == 64 and ref["hist"].shape == (2, 40)
    same(mex.call(8, "vp_corner", None, np.asfortranarray(X), 0.0, 9.0, 0.0, np.asfortranarray(b.T), 0.0, 0.0, 0.5), ref, 8)
    same(mex.call(6, "vp_corner", None, np.asfortranarray(X), 0.0, 9.0, 0.0, np.asfortranarray(b.T), 0.0, 0.0, 0.5), ref, 6)


def test_error_ids(mex):
    from vbmc_amd import vptools as V

    vp = R.make_case("small")[0]
    s = mx_vp(vp)
    Xs, bs = R.small_cut()
    with pytest.raises(MexError) as e:                                                 # the fminbnd branch
        mex.call(1, "vp_corner", None, np.asfortranarray(Xs), 0.0, 1.0, 0.0, np.asfortranarray(bs.T), 0.0, 0.0, 0.5)
    assert e.value.identifier == "vbmc_hip:unsupported" and "pair 1" in e.value.message
    with pytest.raises(MexError) as e:                                                 # kde2d's own default grid
        mex.call(1, "vp_corner", s, None, 67.0, 1.0, 0.0, None, 256.0, 0.0, 0.5)
    assert e.value.identifier == "vbmc_hip:unsupported"
    for args in ((None, None, 67.0, 1.0, 0.0, None, 0.0, 0.0, 0.5),                    # neither a posterior nor a matrix
                 (s, np.zeros((10, 2)), 67.0, 1.0, 0.0, None, 0.0, 0.0, 0.5),          # both
                 (s, None, 0.0, 1.0, 0.0, None, 0.0, 0.0, 0.5),                        # no draws
                 (s, None, 67.0, 1.0, 0.0, np.zeros((2, 3)), 0.0, 0.0, 0.5)):          # bounds of another D
        with pytest.raises(MexError) as e:
            mex.call(1, "vp_corner", *args)
        assert e.value.identifier == "vbmc_hip:usage", (args, e.value)
    Xn = Xs.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(MexError) as e:                                                 # the library's INVALID: its name is the id
        mex.call(1, "vp_corner", None, np.asfortranarray(Xn), 0.0, 1.0, 0.0, None, 16.0, 0.0, 0.5)
    assert e.value.identifier == "vbmc_vp_corner:" and "not finite" in e.value.message
    (xx,) = mex.call(1, "vp_corner", s, None, 67.0, 4.0, 0.0, None, 16.0, 0.0, 0.5)   # the session goes on
    assert np.array_equal(xx, V.vbmc_rnd(vp, 67, True, False, seed=4, nargout=1))

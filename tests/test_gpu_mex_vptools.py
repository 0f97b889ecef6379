"""GPU: the MEX gateway's 'vp_pdf', 'vp_rnd', 'vp_moments' and 'vp_kldiv' commands, executed through the mock of the mx* API
(tests/mock_mex/), return bit for bit what the ctypes mirror (vbmc_amd.vptools) returns for the same call -- both sit on the same entry
points and every call is deterministic given the seed -- on case C of tests/_vptools_ref.py (logit and unbounded variables, scale and
rotation), and an unsupported request comes back as 'vbmc_hip:unsupported', on which the shims fall through."""
import numpy as np
import pytest

from tests import _vptools_ref as T
from tests._mex import MexError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def mx_vp(vp):
    row = lambda v: np.asarray(v, dtype=np.float64).reshape(1, -1)  # noqa: E731
    out = {"D": float(vp["D"]), "K": float(vp["K"]), "mu": np.asfortranarray(vp["mu"]), "sigma": row(vp["sigma"]), "lambda": row(vp["lambda"]), "w": row(vp["w"]),
           "trinfo": None}
    tr = vp.get("trinfo")
    if tr:
        out["trinfo"] = {"lb_orig": row(tr["lb_orig"]), "ub_orig": row(tr["ub_orig"]), "type": row(tr["type"]), "mu": row(tr["mu"]), "delta": row(tr["delta"]),
                         "scale": None if tr["scale"] is None else row(tr["scale"]), "R_mat": None if tr["R_mat"] is None else np.asfortranarray(tr["R_mat"])}
    return out


def test_vp_commands_equal_the_ctypes_calls(mex):
    from vbmc_amd import vptools as V

    for name in ("C", "A"):
        vp = T.make_case(name)
        vp2 = T.sibling(vp, 2)
        s, s2, D = mx_vp(vp), mx_vp(vp2), vp["D"]
        X, I = V.vbmc_rnd(vp, 300, True, True, seed=9)
        Xm, Im = mex.call(2, "vp_rnd", s, 300.0, 1.0, 1.0, np.inf, 9.0)
        assert np.array_equal(Xm, X) and np.array_equal(Im.reshape(-1), I.astype(np.float64))
        Ym, = mex.call(1, "vp_rnd", s, 65.0, 0.0, 0.0, np.inf, 9.0)
        assert np.array_equal(Ym, V.vbmc_rnd(vp, 65, False, False, seed=9, nargout=1))
        for orig, logf, trans, df in ((True, True, False, np.inf), (True, False, False, np.inf), (False, True, False, 5.0), (True, True, True, -5.0)):
            P = Ym if (trans or not orig) else X
            (y,) = mex.call(1, "vp_pdf", s, P, float(orig), float(logf), float(trans), df)
            assert np.array_equal(y.reshape(-1), V.vbmc_pdf(vp, P, orig, logf, trans, df)), (name, orig, logf, trans, df)
        y, dy = mex.call(2, "vp_pdf", s, Ym, 0.0, 1.0, 0.0, np.inf)
        ry, rdy = V.vbmc_pdf(vp, Ym, False, True, nargout=2)
        assert np.array_equal(y.reshape(-1), ry) and np.array_equal(dy, rdy)
        mu, S = mex.call(2, "vp_moments", s, 1003.0, 4.0)
        rmu, rS = V.vbmc_moments(vp, True, 1003, seed=4)
        assert mu.shape == (1, D) and np.array_equal(mu.reshape(-1), rmu) and np.array_equal(S, rS)
        kls, x1, x2 = mex.call(3, "vp_kldiv", s, s2, 1003.0, 4.0)
        rk, r1, r2 = V.vbmc_kldiv(vp, vp2, 1003, seed=4, nargout=3)
        assert kls.shape == (1, 2) and np.array_equal(kls.reshape(-1), rk) and np.array_equal(x1, r1) and np.array_equal(x2, r2)
    vp = T.make_case("C")
    s = mx_vp(vp)
    X = V.vbmc_rnd(vp, 65, True, True, seed=9, nargout=1)
    bad = mx_vp(dict(vp, trinfo=dict(vp["trinfo"], type=np.array([3, 12, 3]))))
    for args in (("vp_pdf", bad, X, 1.0, 1.0, 0.0, np.inf), ("vp_rnd", s, 10.0, 1.0, 0.0, 5.0, 1.0), ("vp_rnd", s, 10.0, 1.0, 2.0, np.inf, 1.0),
                 ("vp_moments", bad, 100.0, 1.0), ("vp_kldiv", s, mx_vp(T.make_case("C", seed=5)), 100.0, 1.0)):
        with pytest.raises(MexError) as e:
            mex.call(1, *args)
        assert e.value.identifier == "vbmc_hip:unsupported", args[0]
    with pytest.raises(MexError) as e:                                                 # the gradient in the original space
        mex.call(2, "vp_pdf", s, X, 1.0, 1.0, 0.0, np.inf)
    assert e.value.identifier == "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:                                                 # vp is not a struct
        mex.call(1, "vp_pdf", 3.0, X, 1.0, 1.0, 0.0, np.inf)
    assert e.value.identifier == "vbmc_hip:usage"
    with pytest.raises(MexError) as e:                                                 # X of another width
        mex.call(1, "vp_pdf", s, X[:, :2], 1.0, 1.0, 0.0, np.inf)
    assert e.value.identifier == "vbmc_hip:usage"
    (y,) = mex.call(1, "vp_pdf", s, X, 1.0, 1.0, 0.0, np.inf)                      # the session goes on
    assert np.array_equal(y.reshape(-1), V.vbmc_pdf(vp, X, True, True))

"""GPU: the MEX gateway's 'gp_surrogate_sample' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for
bit what the ctypes mirror (vbmc_amd.gplite.gplite_sample_device) returns for the same call -- both sit on vbmc_gp_surrogate_sample and
the call is deterministic given the seed --, with and without the noise estimate and the way back to the original space, and an
unsupported request comes back as 'vbmc_hip:unsupported', on which the shim falls through."""
import numpy as np
import pytest

from tests import _gpsample_ref as G
from tests._mex import MexError
from tests.test_gpu_mex_quad import _gp_struct
from tests.test_gpu_mex_vptools import mx_vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def test_gp_surrogate_sample_command_equals_the_ctypes_call(mex):
    from vbmc_amd.gplite import gplite_sample_device

    c = G.build_vp_case("C")
    vp, gp, nz, D = c["vp"], c["gp"], c["noise"], c["D"]
    row = lambda v: np.asarray(v, dtype=np.float64).reshape(1, -1)  # noqa: E731
    noise = {"X_rescaled": np.asfortranarray(nz["X_rescaled"]), "gplengthscale": row(nz["gplengthscale"]), "sn2new": nz["sn2new"].reshape(-1, 1)}
    none = np.zeros((0, 0))
    s = mx_vp(vp)
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    hh = np.uint64(h[0, 0])
    S = float(len(gp["post"]))
    try:
        r = gplite_sample_device(gp, 21, c["LB"], c["UB"], vp=vp, E=2, noise=dict(nz, Nnn=G.NNN), origflag=True, seed=77, spec=3)
        X, out = mex.call(2, "gp_surrogate_sample", hh, s, 21.0, 1.0, row(c["LB"]), row(c["UB"]), noise,
                          {"S": S, "E": 2.0, "Seed": 77.0, "Spec": 3.0, "Nnn": float(G.NNN)})
        assert X.shape == (21, D) and np.array_equal(X, r["X"])
        assert (out["VarThresh"][0, 0], out["sn2_avg"][0, 0]) == (r["VarThresh"], r["sn2_avg"]) and r["sn2_avg"] > 1.0
        assert (out["funccount"][0, 0], out["performed"][0, 0], out["rounds"][0, 0]) == (r["funccount"], r["performed"], r["rounds"])
        # no estimate, the transformed space, a start handed over
        x0 = r["x0"]
        t = gplite_sample_device(gp, 9, c["LB"], c["UB"], x0=x0, E=2, VarThresh=2.5, beta=0.25, thin=2, seed=5)
        (Xt,) = mex.call(1, "gp_surrogate_sample", hh, none, 9.0, 0.0, row(c["LB"]), row(c["UB"]), none,
                         {"S": S, "E": 2.0, "Seed": 5.0, "VarThresh": 2.5, "Beta": 0.25, "Thin": 2.0, "x0": np.asfortranarray(np.transpose(x0, (1, 2, 0)))})
        assert np.array_equal(Xt, t["X"])
        with pytest.raises(MexError) as e:                                             # a transform the library does not accelerate
            bad = dict(s, trinfo=dict(s["trinfo"], type=row([3, 5, 3])))
            mex.call(1, "gp_surrogate_sample", hh, bad, 9.0, 1.0, row(c["LB"]), row(c["UB"]), none, {"S": S, "Seed": 1.0})
        assert e.value.identifier == "vbmc_hip:unsupported"
        with pytest.raises(MexError) as e:                                             # a box of the wrong length
            mex.call(1, "gp_surrogate_sample", hh, s, 9.0, 1.0, row(c["LB"])[:, :-1], row(c["UB"]), none, {"S": S, "Seed": 1.0})
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                             # origflag without a posterior
            mex.call(1, "gp_surrogate_sample", hh, none, 9.0, 1.0, row(c["LB"]), row(c["UB"]), none, {"S": S, "Seed": 1.0})
        assert e.value.identifier not in ("vbmc_hip:unsupported", "vbmc_hip:usage")
        (X2,) = mex.call(1, "gp_surrogate_sample", hh, s, 4.0, 1.0, row(c["LB"]), row(c["UB"]), none, {"S": S, "Seed": 2.0})   # the session goes on
        assert X2.shape == (4, D)
    finally:
        mex.call(0, "gp_free", hh)

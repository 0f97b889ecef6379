"""GPU: the MEX gateway's 'is_setup' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit what the
ctypes mirror returns for the same call (case A of tests/_issetup_ref.py) -- both sit on vbmc_acq_is_setup and the call is deterministic
given the seed or the blocks -- and its state handle is one 'acq_iqr' accepts."""
import numpy as np
import pytest

from tests import _issetup_ref as T
from tests._mex import MexError
from tests.test_gpu_mex_quad import _gp_struct

pytestmark = pytest.mark.gpu
STEP1 = ("Xa1", "lnw1", "fs2a1", "rect_delta", "LB", "UB")


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def test_is_setup_command_equals_the_ctypes_call(mex):
    from vbmc_amd.acq import importance_setup_device

    c, _ = T.run_case("A")
    gp, S, D = c["gp"], c["S"], c["D"]
    row = lambda v: np.asarray(v, dtype=np.float64).reshape(1, -1)  # noqa: E731
    vp = {"mu": np.asfortranarray(c["vp"]["mu"]), "sigma": row(c["vp"]["sigma"]), "lambda": np.asarray(c["vp"]["lambda"], dtype=np.float64).reshape(-1, 1),
          "w": row(c["vp"]["w"])}
    (h,) = mex.call(1, "gp_upload", _gp_struct(gp))
    hh = np.uint64(h[0, 0])
    handles = []
    try:
        for kw, opts in ((dict(seed=77, spec=3), {"Seed": 77.0, "Spec": 3.0, "S": float(S)}),
                         (dict(block=c["B"], uniforms=c["U"], spec=2), {"B": c["B"].reshape(-1, 1), "U": np.asfortranarray(c["U"]), "Spec": 2.0, "S": float(S)})):
            r = importance_setup_device(c["vp"], gp, c["Nvp"], c["Nbox"], c["Nm"], want_state=False, **kw)
            Xa, lnw, fs2a, his, out = mex.call(5, "is_setup", hh, vp, float(c["Nvp"]), float(c["Nbox"]), float(c["Nm"]), opts)
            handles.append(np.uint64(his[0, 0]))
            assert his[0, 0] != 0
            assert np.array_equal(Xa, r["Xa"]) and np.array_equal(lnw, r["lnw"]) and np.array_equal(fs2a, r["fs2a"])
            for k in STEP1:
                assert np.array_equal(out[k].reshape(r[k].shape), r[k]), k
            assert np.array_equal(out["lpdf1"].reshape(-1), r["lpdf1"]) and np.array_equal(out["logp"], r["logp"])
            assert np.array_equal(np.transpose(out["x0"], (2, 0, 1)), r["x0"]) and np.array_equal(out["idx0"], r["idx0"].astype(np.float64))
            assert out["n_bad"][0, 0] == 0 and not np.any(out["bad"])
            assert (out["funccount"][0, 0], out["performed"][0, 0], out["rounds"][0, 0]) == (r["funccount"], r["performed"], r["rounds"])
        # Step 1 alone: the state of the shared points
        r = importance_setup_device(c["vp"], gp, c["Nvp"], c["Nbox"], 0, seed=5, want_state=False)
        Xa, lnw, fs2a, his, out = mex.call(5, "is_setup", hh, vp, float(c["Nvp"]), float(c["Nbox"]), 0.0, {"Seed": 5.0, "S": float(S)})
        handles.append(np.uint64(his[0, 0]))
        assert Xa.size == 0 and his[0, 0] != 0 and np.array_equal(out["lnw1"], r["lnw1"]) and np.array_equal(out["Xa1"], r["Xa1"])
        with pytest.raises(MexError) as e:                                             # no importance points at all
            mex.call(1, "is_setup", hh, vp, 0.0, 0.0, float(c["Nm"]), {"Seed": 1.0, "S": float(S)})
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                             # more points than the importance state holds
            mex.call(1, "is_setup", hh, vp, 200.0, 100.0, float(c["Nm"]), {"Seed": 1.0, "S": float(S)})
        assert e.value.identifier not in ("vbmc_hip:unsupported", "vbmc_hip:usage")
        with pytest.raises(MexError) as e:                                             # vp is not a struct
            mex.call(1, "is_setup", hh, 3.0, 10.0, 10.0, float(c["Nm"]), {"Seed": 1.0, "S": float(S)})
        assert e.value.identifier == "vbmc_hip:usage"
        with pytest.raises(MexError) as e:                                             # a block of the wrong length
            mex.call(1, "is_setup", hh, vp, float(c["Nvp"]), float(c["Nbox"]), float(c["Nm"]), {"B": c["B"][:-1].reshape(-1, 1), "S": float(S)})
        assert e.value.identifier == "vbmc_hip:usage"
        (X2,) = mex.call(1, "is_setup", hh, vp, 10.0, 6.0, 4.0, {"Seed": 2.0, "S": float(S)})      # the session goes on
        assert X2.shape == (4, D, S)
    finally:
        for hi in handles:
            mex.call(0, "is_free", hi)
        mex.call(0, "gp_free", hh)

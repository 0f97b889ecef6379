"""GPU: the MEX gateway's 'slice_sample' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit
what the ctypes mirror returns for the same call -- both sit on vbmc_gp_slice_sample and the chain is deterministic."""
import numpy as np
import pytest

from tests._mex import MexError
from tests.test_gpu_slice import CASES, problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def _call(mex, nlhs, gp, hp, x0, Ns, widths, LB, UB, opts, W, seed, perms, U):
    o = np.array([Ns, opts["Thin"], opts["Burnin"], int(opts["Adaptive"]), W], dtype=np.float64)
    pm = None if perms is None else (perms.T + 1).astype(np.float64)            # Nhyp x sweeps, 1-based as randperm returns them
    Um = None if U is None else np.ascontiguousarray(U).transpose(2, 1, 0)       # (2 + Kmax) x Nhyp x sweeps, column-major
    s2 = None if gp["s2"] is None else gp["s2"].reshape(-1, 1)
    return mex.call(nlhs, "slice_sample", gp["X"], gp["y"].reshape(-1, 1), s2, gp["meanfun"], np.array(gp["noisefun"], dtype=np.float64),
                    {"mu": hp["mu"], "sigma": hp["sigma"], "df": hp["df"]}, LB.reshape(1, -1), UB.reshape(1, -1), x0.reshape(1, -1),
                    widths.reshape(1, -1), widths.reshape(1, -1), o, float(seed), pm, Um)


@pytest.mark.parametrize("ci", [2, 3])
def test_slice_sample_command_equals_the_ctypes_call(mex, ci):
    import vbmc_amd as va

    gp, hp, x0, Ns, widths, LB, UB, opts, perms, U = problem(CASES[ci])
    s, f, _, out = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, uniforms=U, perms=perms, W=4)
    ms, mf, mw, mc = _call(mex, 4, gp, hp, x0, Ns, widths, LB, UB, opts, 4, 0, perms, U)
    assert ms.shape == (Ns, x0.size) and mf.shape == (Ns, 1) and mw.shape == (1, x0.size) and mc.shape == (1, 3)
    assert np.array_equal(ms, s) and np.array_equal(mf[:, 0], f) and np.array_equal(mw[0], out.widths)
    assert [int(v) for v in mc[0]] == [out.funccount, out.performed, out.maxshrink]
    # the device generator keyed by the seed, one output only
    s2, _, _, _ = va.slicesamplebnd_gp(gp, hp, x0, Ns, widths, LB, UB, opts, seed=9, W=2)
    (m2,) = _call(mex, 1, gp, hp, x0, Ns, widths, LB, UB, opts, 2, 9, None, None)
    assert np.array_equal(m2, s2)


def test_slice_sample_errors_are_matlab_ids(mex):
    gp, hp, x0, Ns, widths, LB, UB, opts, perms, U = problem(CASES[0])
    bad = x0.copy()
    bad[1] = UB[1] + 1.0
    with pytest.raises(MexError) as e:
        _call(mex, 1, gp, hp, bad, Ns, widths, LB, UB, opts, 1, 0, perms, U)
    assert e.value.identifier == "slicesamplebnd:start"
    with pytest.raises(MexError) as e:
        _call(mex, 1, dict(gp, meanfun=6), hp, x0, Ns, widths, LB, UB, opts, 1, 0, perms, U)
    assert e.value.identifier == "vbmc_hip:unsupported"

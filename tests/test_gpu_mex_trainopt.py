"""GPU: the MEX gateway's 'gp_train_opt' command, executed through the mock of the mx* API (tests/mock_mex/), returns bit for bit
what the ctypes mirror returns for the same call -- both sit on vbmc_gp_train_optimize and the call is deterministic."""
import numpy as np
import pytest

from tests._mex import MexError
from tests._trainopt_cases import PARITY_NINIT, parity_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    yield m
    assert m.live_arrays() == 0


def _call(mex, nlhs, c, design, Ninit, Nopts, tol, maxit, W, meanfun=None):
    gp, hp = c["gp"], c["hprior"]
    s2 = None if gp["s2"] is None else gp["s2"].reshape(-1, 1)
    prior = None if hp is None else {"mu": hp["mu"], "sigma": hp["sigma"], "df": hp["df"]}
    o = np.array([Ninit, Nopts, tol, maxit, 3000, W], dtype=np.float64)
    return mex.call(nlhs, "gp_train_opt", gp["X"], gp["y"].reshape(-1, 1), s2, gp["meanfun"] if meanfun is None else meanfun,
                    np.array(gp["noisefun"], dtype=np.float64), prior, c["LB"].reshape(1, -1), c["UB"].reshape(1, -1), np.asfortranarray(design), o)


@pytest.mark.parametrize("ci", [1, 3])
def test_gp_train_opt_command_equals_the_ctypes_call(mex, ci):
    import vbmc_amd as va

    c, tol, maxit = parity_case(ci)
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], PARITY_NINIT, seed=3)
    out = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"],
                                   {"Design": design, "Nopts": 2, "TolFun": tol, "MaxIter": maxit, "W": 2})
    hyp, nll, hs, best, wd, cn, pf, ff, fo = _call(mex, 9, c, design, PARITY_NINIT, 2, tol, maxit, 2)
    Nhyp = c["h0"].size
    assert hyp.shape == (Nhyp, 2) and nll.shape == (1, 2) and hs.shape == (Nhyp, 1) and cn.shape == (3, 2) and ff.shape == (1, PARITY_NINIT)
    assert np.array_equal(hyp, out["hyp"]) and np.array_equal(nll[0], out["nll"]) and np.array_equal(hs[:, 0], out["hyp_start"])
    assert int(best[0, 0]) == out["best"] + 1 and np.array_equal(wd[0], out["widths_default"])
    assert [int(v) for v in cn[0]] == list(out["iterations"]) and [int(v) for v in cn[1]] == list(out["funccount"])
    assert [int(v) for v in cn[2]] == list(out["exitflag"]) and int(pf[0, 0]) == out["performed"]
    assert np.array_equal(ff[0], out["fill_fvals"], equal_nan=True) and [int(v) - 1 for v in fo[0]] == list(out["fill_order"])
    # one output only, and the branch without a fill stage: the given column is the start
    o0 = va.gplite_train_optimize(c["gp"], c["h0"], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], {"Ninit": 0, "Nopts": 1, "TolFun": tol, "MaxIter": 5})
    (h0,) = _call(mex, 1, c, c["h0"][None], 0, 1, tol, 5, 0)
    assert np.array_equal(h0, o0["hyp"])


def test_gp_train_opt_errors_are_matlab_ids(mex):
    import vbmc_amd as va

    c, tol, maxit = parity_case(1)
    design = va.fminfill_design(c["h0"][None], c["LB"], c["UB"], c["PLB"], c["PUB"], c["hprior"], PARITY_NINIT, seed=3)
    with pytest.raises(MexError) as e:
        _call(mex, 1, c, design, PARITY_NINIT, 2, tol, maxit, 1, meanfun=6)
    assert e.value.identifier == "vbmc_hip:unsupported"
    with pytest.raises(MexError) as e:
        _call(mex, 1, c, design, PARITY_NINIT - 1, 2, tol, maxit, 1)
    assert e.value.identifier == "vbmc_hip:usage"
    (h,) = _call(mex, 1, c, design, PARITY_NINIT, 2, tol, 3, 1)          # the gateway's context is still usable
    assert h.shape == (c["h0"].size, 2)

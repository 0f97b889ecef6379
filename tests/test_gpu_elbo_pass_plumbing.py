"""Host plumbing of the blocking ELBO call (vbmc_amd/csrc/elbo_pass.h): the pooled blocks behind the per-hyper-sample outputs live side by
side without touching each other, and a call the plan refuses leaves nothing behind on the context."""
import ctypes as C

import numpy as np
import pytest

from tests._cases import synth_problem

pytestmark = pytest.mark.gpu

PER_SAMPLE = ("G_s", "varG_s", "dG_s", "dvarG_s", "dvarG")


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


@pytest.fixture(scope="module")
def prob(va):
    D, N, K, S, R = 2, 12, 3, 3, 2
    p = synth_problem(11, D, N, K, S)
    gp = va.gplite_post(p["hyp"], p["X"], p["y"], 1, p["meanfun"])
    vp = va.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    theta = np.concatenate([p["mu"].reshape(-1, order="F"), np.log(p["sigma"]), np.log(p["lam"]), p["eta"]])
    thetas = np.asfortranarray(theta[:, None] + 0.05 * np.random.default_rng(11).standard_normal((theta.size, R)))
    return gp, vp, thetas


def test_per_sample_outputs_requested_together_equal_each_requested_alone(va, prob):
    """G_s, varG_s, dG_s, dvarG_s and dvarG in ONE vbmc_elbo_batch call (compute_var = 2, gradient): every pooled block of the call is
    live at once, and each output has the bits of the call that asks for it alone."""
    gp, vp, thetas = prob
    call = lambda outs: va.negelcbo_batch(thetas, 0.0, vp, gp, 40, True, 2, seed=5, outputs=outs)
    together = call(PER_SAMPLE + ("F", "dF"))
    for name in PER_SAMPLE:
        alone = call((name,))
        assert set(alone) == {name}
        assert together[name].shape == alone[name].shape and np.all(np.isfinite(alone[name]))
        assert np.array_equal(together[name], alone[name]), name
    assert np.array_equal(together["F"], call(("F",))["F"])


def test_varG_s_without_a_variance_is_refused_before_anything_is_enqueued(va, prob):
    """varG_s with compute_var = 0: INVALID with its message, and the context is as it was -- the next valid call returns the bits a
    fresh context returns, and the pipeline's slot 0 works."""
    from vbmc_amd import elbo as E
    from vbmc_amd._lib import VbmcHipError, ptr

    gp, vp, thetas = prob
    T, R = thetas.shape
    S = len(gp["post"])
    eng = E.Engine(0)
    a, keep, _ = E._build_args(thetas=thetas, beta=0.0, vp=vp, gp=gp, Ns=40, compute_grad=True, compute_var=0, thetabnd=None,
                               separate_K=False, eps=None, eps_device_ptr=None, eps_shared=False, seed=5, engine=eng)
    F = np.empty(R)
    varGs = np.empty((S, R), order="F")
    a.F, a.varG_s = ptr(F), ptr(varGs)
    dgp = eng.device_gp(gp)
    st = eng.ctx.lib.vbmc_elbo_batch(eng.ctx.h, dgp.h, C.byref(a))
    with pytest.raises(VbmcHipError, match="varG_s needs compute_var != 0") as ei:
        eng.ctx.check(st)
    assert st == 1 and ei.value.status == 1     # VBMC_ERR_INVALID
    valid = lambda e: va.negelcbo_batch(thetas, 0.0, vp, gp, 40, True, 0, seed=5, engine=e, outputs=("F", "dF", "G_s"))
    after, fresh = valid(eng), valid(E.Engine(0))
    for name in ("F", "dF", "G_s"):
        assert np.array_equal(after[name], fresh[name]), name
    obj = va.PreparedObjective(T, R, 0, vp, gp, 40, 0, None, engine=eng)
    Fb, dFb = (x.copy() for x in obj(thetas, seed=5))
    obj.submit(thetas, seed=5, slot=0)
    Fs, dFs = obj.collect(0)
    assert np.array_equal(Fs, Fb) and np.array_equal(dFs, dFb)
    assert np.array_equal(Fb, fresh["F"]) and np.array_equal(dFb, fresh["dF"])

"""GPU: every launch form of the variance of the expected log joint (vbmc_amd/csrc/elbo_pass.h: Pass::variance) against the
extended-precision restatement tests/_var_ref.py, on the cases of tests/_var_cases.py -- mixtures whose components overlap, each shape the
smallest that reaches its edge.

Every case asserts, through the reporting hook ``Context.last_variance`` (vbmc_ctx_last_variance), that the pass it ran took the form it
is about (product with inv(L') or substitution, which substitution and how wide, which Gram kernel, the dynamic LDS of k_var_sample and
k_var_final); asserts the power conditions from the reference alone (in every 16 x 16 tile of the upper triangle at least 0.15 of the
off-diagonal pairs have a data term and a prior term above 1e-3 of their diagonals'; no J_kk at the clamp; every block of dvarF has a
data term; a case with vp.delta moves by 1e4 bounds without it); and compares each restart's column with its own reference: J_sjk,
varG, varGss, varG_s, and with a gradient dvarG and dvarG_s block by block.

Tolerance.  The measures of tests/_var_ref.py are in units of u = 2^-53 of the magnitudes added up, entry by entry, with no floor.  The
float64 oracle's worst error, as measured, is E_REF_J / E_REF_VAR / E_REF_DVAR (tests/test_var_restatement.py); the device gets
DEVICE_FACTOR = 32 times that, for the reasons of tests/test_gpu_pred_forms.py and more: its exponential is the table form in all N
terms, its sums run in MFMA and wave order, and the product with an explicit inverse stands in for a substitution.  DESIGN.md
("Variance: launch forms and accuracy") has the figures per form."""
import numpy as np
import pytest

from tests import _var_cases as C
from tests import _var_ref as V
from tests.test_var_restatement import BOUND_DVAR, BOUND_J, BOUND_VAR, delta_matters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


def run_case(va, name, cols=None, **kw):
    """-> (outputs of one pass over the case's restarts (or the columns ``cols``), its launch record)"""
    c, d = C.CASES[name], C.case_inputs(name)
    th = d["thetas"] if cols is None else np.asfortranarray(d["thetas"][:, cols])
    if c["grad"]:
        out = va.negelcbo_batch(th, 0.0, d["vp"], d["gp"], 0, True, c["cv"], jacobian_flag=c["jac"],
                                outputs=("G", "varG", "varGss", "dvarG", "G_s", "varG_s", "dvarG_s"), **kw)
    else:
        out = va.negelcbo_batch(th, 0.0, d["vp"], d["gp"], 0, False, c["cv"], separate_K=True,
                                outputs=("G", "varG", "varGss", "I_sk", "J_sjk", "G_s", "varG_s"), **kw)
    return out, va.default_engine().ctx.last_variance()


def errors(name, out, r, ref):
    """the case's compared outputs of column r of ``out`` in the restatement's units -> dict"""
    c = C.CASES[name]
    e = {"varG_s": V.err_units(out["varG_s"][:, r], ref.varF_s, ref.varF_mag), "varG": V.err_units(out["varG"][r], ref.varG, ref.varG_mag)}
    if c["S"] > 1:
        e["varGss"] = V.err_units(out["varGss"][r], ref.varGss, ref.varGss_mag)
    if not c["grad"]:
        e["J"] = V.err_J(out["J_sjk"][:, :, :, r], ref, c["cv"])
    else:
        for k, v in V.err_dvar_blocks(out["dvarG"][:, r], ref.dvarF, ref.dvarF_mag, ref.sizes).items():
            e["dvarG " + k] = v
        for k, v in V.err_dvar_blocks(out["dvarG_s"][:, :, r], ref.dvarF_s, ref.dvarF_s_mag, ref.sizes).items():
            e["dvarG_s " + k] = v
    return e


def bound_of(key):
    return BOUND_J if key == "J" else (BOUND_DVAR if key.startswith("dvarG") else BOUND_VAR)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_form_against_restatement(va, name):
    c, d = C.CASES[name], C.case_data(name)
    out, rec = run_case(va, name)
    print(name, rec)
    C.check_form(name, rec)
    C.check_mixed(name, d["gp"])
    if c["delta"]:
        delta_matters(name)
    for r, ref in enumerate(d["refs"]):
        V.assert_power(ref, c["cv"], c["grad"], "%s, restart %d" % (name, r))
        if c["S"] == 1:
            assert out["varGss"][r] == 0.0
        e = errors(name, out, r, ref)
        print("%-18s r%d device e: %s" % (name, r, "  ".join("%s %.1f" % kv for kv in e.items())))
        over = {k: (v, bound_of(k)) for k, v in e.items() if not v <= bound_of(k)}
        assert not over, (name, r, over)


@pytest.mark.parametrize("name", ["restarts_full", "restarts_diag"])
def test_one_restart_alone_gives_its_column(va, name):
    """R = 1 on a column: the outputs of the variance stage alone (J_sjk, varG_s, dvarG_s) carry that column's bits whatever the batch;
    as a declared share of the batch (restart_offset, plan_restarts: the launch shapes of the whole batch) every output does"""
    c = C.CASES[name]
    out, _ = run_case(va, name)
    stage = ("varG_s", "dvarG_s") if c["grad"] else ("varG_s", "J_sjk")
    for r in range(c["R"]):
        one, rec = run_case(va, name, cols=[r])
        C.check_form(name, rec)
        for k in stage:
            assert np.array_equal(one[k][..., 0], out[k][..., r]), (name, r, k)
        share, _ = run_case(va, name, cols=[r], restart_offset=r, plan_restarts=c["R"])
        for k in share:
            assert np.array_equal(share[k][..., 0], out[k][..., r]), (name, r, k)

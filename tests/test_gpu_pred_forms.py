"""GPU: every launch form of the prediction (vbmc_amd/csrc/gp_pred.h: pred_forms) against the extended-precision restatement
tests/_pred_ref.py, on the cases of tests/_pred_cases.py -- each the smallest shape that reaches its form.

Every case asserts, through the reporting hook ``vbmc_amd.gplite.pred_plan`` (vbmc_pred_plan), that it reached the form it is about;
asserts the power condition (the points see the data: without it fmu is the mean function and fs2 is sf2 whatever the kernels compute);
and compares fmu, fs2, ys2 (F, varF for the quadrature) per hyper-sample with the restatement.

Tolerance.  The measures of tests/_pred_ref.py are in units of u = 2^-53 of the magnitudes added up.  The float64 oracle's worst error
over all cases, as measured, is E_REF_V / E_REF_M (tests/test_pred_restatement.py); the device gets 32 times that: its
exponential is the table form (<= 2 ulp) in all N terms, its sums run in MFMA and wave order, and its distances come, like the
oracle's, from |a|^2 + |b|^2 - 2 a.b on centred inputs.  DESIGN.md ("Prediction: launch forms and accuracy") has the figures per form.

The two-kernel form is switched on by VBMC_PRED_FUSED=0, read once per process: those cases run in one child process
(tests/_pred_forms_child.py) that writes one .npz, compared here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _pred_cases as C
from tests import _pred_ref as P
from tests.test_pred_restatement import DEVICE_FACTOR, E_REF_M, E_REF_V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_V, BOUND_M = DEVICE_FACTOR * E_REF_V, DEVICE_FACTOR * E_REF_M
ONE_PROCESS = sorted(n for n, c in C.CASES.items() if not c["two_kernel"])
TWO_KERNEL = sorted(n for n, c in C.CASES.items() if c["two_kernel"])


@pytest.fixture(scope="module")
def va():
    import vbmc_amd

    return vbmc_amd


@pytest.fixture(scope="module")
def num_cu(va):
    from vbmc_amd import gplite

    return gplite.pred_plan(C.case_data("nstar_1")["gp"], 1)["num_cu"]


def compare_pred(name, d, outs):
    ymu, ys2, fmu, fs2 = outs
    ref = d["ref"]
    eM, eV, eY = P.err_fmu(fmu, ref), P.err_fs2(fs2, ref), P.err_fs2(ys2, ref, field="ys2")
    print("%-20s device e: fmu %8.1f  fs2 %8.1f  ys2 %8.1f   (bounds %g, %g)" % (name, eM, eV, eY, BOUND_M, BOUND_V))
    assert np.array_equal(ymu, fmu) and np.all(np.asarray(fs2) >= 0.0)
    assert eM <= BOUND_M and eV <= BOUND_V and eY <= BOUND_V, (name, eM, eV, eY)


def averaged_reference(ref):
    """gplite_pred.m:154-165 on the restatement -> (fbar, fs2 averaged, and the error either may carry when every per-sample value
    is within its bound: d(vf) <= sum_s 2 |fmu_s - fbar| (d fmu_s + d fbar) / (S - 1))"""
    S = ref.fmu.shape[1]
    fs2c = np.maximum(ref.fs2, 0)
    fbar = np.sum(ref.fmu, axis=1) / S
    vf = np.sum((ref.fmu - fbar[:, None]) ** 2, axis=1) / (S - 1)
    dM = BOUND_M * P.U * ref.fmag
    tolM = np.sum(dM, axis=1) / S
    tolV = BOUND_V * P.U * np.sum(ref.kss[None, :] + ref.vmag, axis=1) / S + np.sum(2 * np.abs(ref.fmu - fbar[:, None]) * (dM + tolM[:, None]), axis=1) / (S - 1)
    return fbar, np.sum(fs2c, axis=1) / S + vf, tolM, tolV


@pytest.mark.parametrize("name", ONE_PROCESS)
def test_form_against_restatement(va, num_cu, name):
    from vbmc_amd import gplite

    c, d = C.CASES[name], C.case_data(name, num_cu)
    gp, Xs, ref = d["gp"], d["Xs"], d["ref"]
    plan = gplite.pred_plan(gp, Xs.shape[0], quad=c["quad"])
    print(name, plan)
    C.check_form(name, plan)
    P.assert_power(ref, name)
    C.check_mixed(name, gp)
    if c["quad"]:
        from tests.test_gpu_quad import _conditioned

        assert _conditioned(gp, Xs, d["sigma"]) < 1e-10
        F, V = va.gplite_quad(gp, Xs, d["sigma"], True)
        eM, eV = P.err_fmu(F, ref), P.err_fs2(V, ref, clamp=P.EPS)
        print("%-20s device e: F   %8.1f  varF %8.1f   (bounds %g, %g)" % (name, eM, eV, BOUND_M, BOUND_V))
        assert np.all(V >= P.EPS) and eM <= BOUND_M and eV <= BOUND_V, (name, eM, eV)
        return
    # (RS > 1: every workgroup of a unit computes fmu's data term and rs = 0 alone writes it; k_pred_final adds it to the mean once)
    compare_pred(name, d, va.gplite_pred(gp, Xs, d["ys"], d["s2s"], True))
    if name == "nstar_17":     # the averaged outputs of one case
        ymu_a, ys2_a, fmu_a, fs2_a = va.gplite_pred(gp, Xs, d["ys"], d["s2s"], False)
        fbar, fs2bar, tolM, tolV = averaged_reference(ref)
        assert np.array_equal(ymu_a, fmu_a)
        assert np.all(np.abs(fmu_a - fbar) <= tolM) and np.all(np.abs(fs2_a - fs2bar) <= tolV)
        assert np.all(np.abs(ys2_a - (fs2bar + np.sum(ref.sn2s, axis=1) / c["S"])) <= tolV)


@pytest.fixture(scope="module")
def two_kernel_run(tmp_path_factory):
    """one fresh python child with VBMC_PRED_FUSED=0 runs every two-kernel case; nothing is started after a failure"""
    out = str(tmp_path_factory.mktemp("pred_forms") / "two_kernel.npz")
    env = dict(os.environ, VBMC_PRED_FUSED="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests._pred_forms_child", out], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert r.returncode == 0 and "PRED-FORMS-CHILD-OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", TWO_KERNEL)
def test_two_kernel_form_against_restatement(two_kernel_run, name):
    d = C.case_data(name)
    plan = json.loads(str(two_kernel_run["plan_" + name]))
    print(name, plan)
    C.check_form(name, plan)
    C.check_mixed(name, d["gp"])
    P.assert_power(d["ref"], name)
    compare_pred(name, d, [two_kernel_run[k + "_" + name] for k in ("ymu", "ys2", "fmu", "fs2")])


@pytest.mark.parametrize("name", ["acqviqr", "acqimiqr"])
@pytest.mark.parametrize("shape", C.IQR_SHAPES)
def test_two_kernel_form_through_the_iqr_functions(va, shape, name):
    """the IQR acquisition functions read the cross-kernel matrix: k_pred_ks + k_gp_pred without the switch.  Test and importance points
    near the data, so that the cross term Ks' Ctmp is there; the comparison and its tolerance are those of
    tests/test_gpu_random_shapes._acquisition_case."""
    from vbmc_amd import gplite

    D, N, S, Na = shape
    d = C.iqr_case_data(shape)
    gp, Xs = d["gp"], d["Xs"]
    plan = gplite.pred_plan(gp, Xs.shape[0], want_ks=True)
    assert plan["fused"] == 0 and plan["slab"] == 0 and plan["QS"] == (D + 3) // 4, plan
    P.assert_power(d["ref_s"], "test points")
    P.assert_power(d["ref_a"], "importance points")
    assert d["cross_share"] >= 0.5
    ref, _, vtot = R.acqwrapper_vbmc(Xs, d["vp"], gp, d["st_o"][name], name)
    acq = va.acqwrapper_vbmc(Xs, d["vp"], gp, d["st_d"][name], False, name + "_vbmc", None)
    sf2 = np.exp(2 * gp["post"][0]["hyp"][D])
    ok = np.isfinite(ref) & (vtot > 1e-7 * sf2)
    assert np.mean(ok) >= P.POWER_OK
    rt = 1e-7 + 1e-11 * sf2 / np.maximum(vtot[ok], 1e-300)
    print(shape, name, "worst / allowed %.2e" % np.max(np.abs(acq[ok] - ref[ok]) / (rt * (1 + np.abs(ref[ok])))))
    assert np.all(np.abs(acq[ok] - ref[ok]) < rt * (1 + np.abs(ref[ok]))), (shape, name)

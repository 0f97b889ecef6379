"""CPU check beside tests/test_lane_build.py: the quadrature forms of the prediction kernels (vbmc_amd/csrc/gp_pred_kernels.h) -- k_quad_fused<QS, PT>
for every (QS, PT) the host may launch, PT <= PREDF_PT_FOR_QS(QS), and k_quad_ks<QS> -- compile for gfx950 with no spilled vector registers and
no private segment (the criterion of tests/test_lane_build.py), within the register budget of the prediction forms they share a body with."""
from tests import _abi



def test_quadrature_kernels_do_not_spill(tmp_path):
    combos = [(q, p) for q in range(1, 9) for p in range(1, (3 if q <= 3 else (2 if q <= 5 else 1)) + 1)]
    inst = ["template __global__ void k_quad_fused<%d, %d>(PredArgs, const double*, const double*, const double*, double*, double*, int);" % c for c in combos]
    inst += ["template __global__ void k_quad_ks<%d>(PredArgs, const double*, const double*, const double*, double*, double*);" % q for q in range(1, 9)]
    kernels, _ = _abi.kernel_meta("gp_pred_kernels.h", inst, r"k_quad_[a-z]+$", tmp_path, flags=("-Wno-pass-failed",))
    seen = {"k_quad_fused": 0, "k_quad_ks": 0, "k_quad_prep": 0, "k_quad_final": 0}
    for k in kernels:
        assert _abi.no_scratch(k), k
        seen[k["name"]] += 1
    assert seen == {"k_quad_fused": len(combos), "k_quad_ks": 8, "k_quad_prep": 1, "k_quad_final": 1}, seen

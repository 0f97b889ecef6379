"""CPU check on the small-class entropy kernels (vbmc_amd/csrc/entropy_lane.h): every instantiation k_entropy_lane<DT, KP, grad>
compiles for gfx950 with NO spilled registers and no private segment.  A build of DT = 12, KP = 14 that spilled 87 registers
returned wrong, run-to-run different sums on the GPU (round 6); the register budget per instantiation (ENT_LANE_OCC) is what keeps
them at zero, and this test is what keeps that true."""
import os
from concurrent.futures import ThreadPoolExecutor

from tests import _abi



def test_no_lane_kernel_spills(tmp_path):
    def compile_one(dt):
        return _abi.kernel_meta("ent_lane_inst.hip", (), r"k_entropy_lane$", os.path.join(str(tmp_path), "dt%d" % dt),
                                flags=("-fPIC", "-Wno-pass-failed", "-DDT_VALUE=%d" % dt))[0]

    with ThreadPoolExecutor(max_workers=6) as ex:
        units = list(ex.map(compile_one, (2, 4, 6, 8, 10, 12)))
    seen = 0
    for kernels in units:
        for k in kernels:
            assert k["mangled"].endswith("Ev7EntArgs") and len(k["targs"]) == 3, k["mangled"]      # k_entropy_lane<DT, KP, grad>(EntArgs)
            assert _abi.no_scratch(k), (k["targs"], k["vgpr_spill_count"], k["private_segment_fixed_size"], k["vgpr_count"])
            seen += 1
    assert seen == (4 * 8 + 5 + 4) * 2, seen          # DT = 2..8: KP = 2..16; DT = 10: KP <= 10; DT = 12: KP <= 8


def test_fused_prediction_kernel_does_not_spill(tmp_path):
    """k_pred_fused<QS, PT> (vbmc_amd/csrc/gp_pred_kernels.h) for every (QS, PT) the host may launch -- PT <= PREDF_PT_FOR_QS(QS) -- compiles
    without spilled registers: the resident-tile count is chosen so (three tiles at D <= 12, two up to 20, one beyond)."""
    combos = [(q, p) for q in range(1, 9) for p in range(1, (3 if q <= 3 else (2 if q <= 5 else 1)) + 1)]
    inst = ["template __global__ void k_pred_fused<%d, %d>(PredArgs, const double*, const double*, const double*, double*, double*, int);" % c for c in combos]
    kernels, _ = _abi.kernel_meta("gp_pred_kernels.h", inst, r"k_pred_fused$", tmp_path, flags=("-Wno-pass-failed",))
    seen = 0
    for k in kernels:
        assert len(k["targs"]) == 2 and _abi.no_scratch(k), k
        seen += 1
    assert seen == len(combos), (seen, len(combos))

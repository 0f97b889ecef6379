"""CPU check beside tests/test_lane_build.py: the quadrature forms of the prediction kernels (vbmc_amd/csrc/gp_pred_kernels.h) -- k_quad_fused<QS, PT>
for every (QS, PT) the host may launch, PT <= PREDF_PT_FOR_QS(QS), and k_quad_ks<QS> -- compile for gfx950 with no spilled vector registers and
no private segment (the criterion of tests/test_lane_build.py), within the register budget of the prediction forms they share a body with."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_quadrature_kernels_do_not_spill(tmp_path):
    src = os.path.join(str(tmp_path), "qf.hip")
    combos = [(q, p) for q in range(1, 9) for p in range(1, (3 if q <= 3 else (2 if q <= 5 else 1)) + 1)]
    with open(src, "w") as f:
        f.write('#include "%s/gp_pred_kernels.h"\n' % CSRC)
        for q, p in combos:
            f.write("template __global__ void k_quad_fused<%d, %d>(PredArgs, const double*, const double*, const double*, double*, double*, int);\n" % (q, p))
        for q in range(1, 9):
            f.write("template __global__ void k_quad_ks<%d>(PredArgs, const double*, const double*, const double*, double*, double*);\n" % q)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "qf.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "qf-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {"k_quad_fused": 0, "k_quad_ks": 0, "k_quad_prep": 0, "k_quad_final": 0}
    for m in re.finditer(r"\.name:\s+_Z\d+(k_quad_[a-z]+)(?:ILi\d+E(?:Li\d+E)?Ev)?8PredArgs\S*\n(.*?)\.wavefront_size", asm, re.S):
        meta = m.group(2)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0, m.group(0)[:80]
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0, m.group(0)[:80]
        seen[m.group(1)] += 1
    assert seen == {"k_quad_fused": len(combos), "k_quad_ks": 8, "k_quad_prep": 1, "k_quad_final": 1}, seen

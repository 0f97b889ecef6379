"""CPU check on the slice sampler's kernels: k_slice_propose and k_slice_decide (vbmc_amd/csrc/slice_kernels.h) and k_gpobj_retry
(gpobj_kernels.h, which it includes) compile for gfx950 with no spilled registers and no private segment (the decide kernel keeps
the chain's scalars in registers across its whole body; a spill there would put the sequential tail of every round through scratch
memory)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_slice_propose", "k_gpobj_retry", "k_slice_decide")


def test_slice_kernels_do_not_spill(tmp_path):
    src = os.path.join(str(tmp_path), "sl.hip")
    with open(src, "w") as f:
        f.write('#include "%s/slice_kernels.h"\n' % CSRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "sl.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "sl-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+_Z(\d+)(k_(?:slice|gpobj)_\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name, meta = m.group(2)[: int(m.group(1))], m.group(3)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        assert spill == 0 and sspill == 0 and priv == 0, (name, spill, sspill, priv)
        seen.add(name)
    assert seen == set(KERNELS), seen


def test_slice_sources_use_no_inline_assembly():
    for name in ("slice_kernels.h", "gpobj_kernels.h"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "asm" not in re.sub(r"//.*", "", txt), name

"""CPU check: every header and every ABI file under vbmc_amd/csrc says what it depends on.  Each of them parses for gfx950 as the only
#include of a translation unit, the fourteen ABI files parse in the reverse of vbmc_hip.hip's order, no file but vbmc_hip.hip includes a
.hip file, and the old umbrella header gp_kernels.h is gone.  One parse of host and device per file, no code generation."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "abi_*.hip")))


def _parses(tmp_path, includes):
    src = os.path.join(str(tmp_path), "unit.hip")
    with open(src, "w") as f:
        for name in includes:
            f.write('#include "%s/%s"\n' % (CSRC, name))
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("name", FILES)
def test_file_parses_alone(tmp_path, name):
    _parses(tmp_path, [name])


def test_abi_files_parse_in_reverse_order(tmp_path):
    unit = re.findall(r'#include "(abi_\w+\.hip)"', open(os.path.join(CSRC, "vbmc_hip.hip")).read())
    assert len(unit) == 14 and sorted(unit) == [n for n in FILES if n.endswith(".hip")], unit
    _parses(tmp_path, unit[::-1])


def test_only_the_unit_includes_hip_files():
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(path) == "vbmc_hip.hip" or not os.path.isfile(path):
            continue
        hit = re.findall(r'^\s*#\s*include\s*["<][^">]*\.hip[">]', open(path).read(), re.M)
        assert not hit, (os.path.basename(path), hit)


def test_umbrella_header_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "gp_kernels.h"))
    assert len(FILES) > 30 and "gp_factor_kernels.h" in FILES and "parity_rng.h" in FILES

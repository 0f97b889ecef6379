"""CPU check on the slice sampler's kernels: k_slice_propose and k_slice_decide (vbmc_amd/csrc/slice_kernels.h) and k_gpobj_retry
(gpobj_kernels.h, which it includes) compile for gfx950 with no spilled registers and no private segment (the decide kernel keeps
the chain's scalars in registers across its whole body; a spill there would put the sequential tail of every round through scratch
memory)."""
import os
import re

from tests import _abi

CSRC = _abi.CSRC
KERNELS = ("k_slice_propose", "k_gpobj_retry", "k_slice_decide")


def test_slice_kernels_do_not_spill(tmp_path):
    kernels, _ = _abi.kernel_meta("slice_kernels.h", (), r"k_(slice|gpobj)_", tmp_path)
    seen = set()
    for k in kernels:
        assert _abi.no_scratch(k) and k["sgpr_spill_count"] == 0, k
        seen.add(k["name"])
    assert seen == set(KERNELS), seen


def test_slice_sources_use_no_inline_assembly():
    for name in ("slice_kernels.h", "gpobj_kernels.h"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "asm" not in re.sub(r"//.*", "", txt), name

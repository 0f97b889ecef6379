"""CPU: the form table of the matrix-core entropy kernel (vbmc_amd/csrc/entropy_mfma.h: EntForm).  A host-only program includes the header
itself and prints one line of EntForm members for every class that `dispatch` in ent_mfma_inst.hip can reach: QS = 1..9, its 27
(KT, HV, TL) cases, and per case the variants launch_kt chooses between (value / gradient, block-sparse, log-joint role, device-RNG,
walking), each under the guard the launcher uses (ent_mfma_role_inst, ent_mfma_walk_inst).  The structural invariants are static_asserts
inside EntForm -- the program compiling is their test; here the table is held against the restatements the GPU tests carry (sl_class of
tests/test_gpu_entropy_sample_layout.py, the PM class of tests/test_gpu_entropy_sign_pair.py) and against the launcher's arithmetic."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not found")

FIELDS = ("QS KT GRAD SPARSE HV TL CO EM WALK NPV DP SL EVL PM GP2 NG C2 VBL VBR EPF STAG TQ TWO RNG_CALL WAVES PRIO YXN DYN_LDS").split()

PROGRAM = r"""
#include <cstdio>
#include "entropy_mfma.h"

template <int QS, int KT, bool GRAD, bool SPARSE, int HV = 1, int TL = 0, bool CO = false, bool EM = true, bool WALK = false>
static void row() {
  using F = EntForm<QS, KT, GRAD, SPARSE, HV, TL, CO, EM, WALK>;
  std::printf("%d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu\n", QS, KT, (int)GRAD, (int)SPARSE, HV, TL,
              (int)CO, (int)EM, (int)WALK, F::NPV, F::DP, (int)F::SL, (int)F::EVL, (int)F::PM, (int)F::GP2, F::NG, (int)F::C2, (int)F::VBL, F::VBR,
              (int)F::EPF, (int)F::STAG, (int)F::TQ, (int)F::TWO, (int)F::RNG_CALL, F::WAVES, (int)F::PRIO, F::YXN, (size_t)F::DYN_LDS);
}

// the variants launch_kt<KT, HV, TL> of ent_mfma_inst.hip chooses between
template <int QS, int KT, int HV, int TL = 0>
static void cls() {
  if constexpr (ent_mfma_role_inst(QS, HV)) row<QS, KT, true, false, 1, TL, true>();
  if constexpr (ent_mfma_walk_inst(QS, KT, HV)) {
    row<QS, KT, true, false, 1, TL, false, false, true>();
    row<QS, KT, true, false, 1, TL, false, false>();
  }
  if constexpr (HV == 1 && TL == 0) {
    row<QS, KT, true, true, 1>();
    row<QS, KT, false, true, 1>();
  }
  row<QS, KT, true, false, HV, TL>();
  row<QS, KT, false, false, HV, TL>();
}

// the 27 cases of dispatch
template <int QS>
static void unit() {
  cls<QS, 1, 1>(); cls<QS, 2, 1>(); cls<QS, 3, 1>(); cls<QS, 4, 1>();
  cls<QS, 1, 1, 1>(); cls<QS, 2, 1, 1>(); cls<QS, 3, 1, 1>();
  cls<QS, 2, 2, 1>(); cls<QS, 3, 2, 1>(); cls<QS, 2, 4, 1>(); cls<QS, 3, 4, 1>();
  cls<QS, 1, 1, 2>(); cls<QS, 2, 1, 2>(); cls<QS, 3, 1, 2>();
  cls<QS, 2, 2, 2>(); cls<QS, 3, 2, 2>(); cls<QS, 2, 4, 2>(); cls<QS, 3, 4, 2>();
  cls<QS, 2, 2>(); cls<QS, 3, 2>(); cls<QS, 4, 2>();
  cls<QS, 2, 4>(); cls<QS, 3, 4>(); cls<QS, 4, 4>();
  cls<QS, 3, 8>(); cls<QS, 4, 8>();
}

int main() {
  unit<1>(); unit<2>(); unit<3>(); unit<4>(); unit<5>(); unit<6>(); unit<7>(); unit<8>(); unit<9>();
  return 0;
}
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    d = tmp_path_factory.mktemp("entforms")
    src, exe = str(d / "forms.hip"), str(d / "forms")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-Wno-unused-value", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]      # (EntForm's static_asserts are checked here)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = [dict(zip(FIELDS, map(int, line.split()))) for line in out.splitlines()]
    assert all(len(line.split()) == len(FIELDS) for line in out.splitlines())
    return rows


def test_every_dispatch_class_is_printed(forms):
    # 26 case labels in dispatch's switch plus the default; per QS the classes below
    keys = {tuple(f[k] for k in FIELDS[:9]) for f in forms}
    assert len(keys) == len(forms)
    assert {f["QS"] for f in forms} == set(range(1, 10))
    cases = {(f["KT"], f["HV"], f["TL"]) for f in forms if not f["SPARSE"] and not f["CO"] and f["EM"]}
    assert len(cases) == 26
    for qs in range(1, 10):
        mine = [f for f in forms if f["QS"] == qs]
        assert sum(f["CO"] for f in mine) == (10 if qs <= 8 else 0)             # the ten single-wave classes carry the role up to D = 30
        assert sum(f["WALK"] for f in mine) == (9 if qs <= 4 else 0)            # KT <= 3 on one wave, any tail
        assert sum(f["SPARSE"] for f in mine) == 8                              # KT = 1..4, value and gradient


def test_sample_layout_table_equals_the_gpu_tests_restatement(forms):
    from tests.test_gpu_entropy_sample_layout import sl_class

    n = 0
    for f in forms:
        if f["GRAD"] and not f["SPARSE"] and f["HV"] == 1 and not f["WALK"]:
            assert bool(f["SL"]) == sl_class(f["QS"], f["KT"], f["TL"]), f
            n += 1
    assert n >= 9 * 10
    assert not any(f["SL"] for f in forms if f["WALK"] or not f["GRAD"] or f["HV"] > 1)


def test_sign_pair_class_and_the_implications(forms):
    for f in forms:
        assert bool(f["PM"]) == bool(f["SL"] and f["QS"] == 3 and f["KT"] == 3 and f["TL"] == 1 and not f["SPARSE"]), f
        assert not f["PM"] or f["SL"]
        assert not f["SL"] or f["NPV"] == 1
        assert not (f["GP2"] and f["SL"]), f
        assert not f["TQ"] or f["GP2"], f
        assert f["VBR"] <= f["KT"] * 4 * f["NPV"], f
        assert f["WAVES"] in (1, 2, 3), f
        assert f["NPV"] == (4 * f["QS"] + 15) // 16 and f["DP"] == 4 * f["QS"]
    assert any(f["PM"] for f in forms)


def test_dynamic_lds_after_the_parameter_block(forms):
    table = 1024 * 8
    for f in forms:
        if f["HV"] > 1:
            assert f["DYN_LDS"] == table + f["HV"] * f["NPV"] * 4 * 64 * 8, f
        else:
            assert f["DYN_LDS"] == table, f
    # the launcher reads the size off the value kernel of the class: every variant of a class has the same
    by_class = {}
    for f in forms:
        by_class.setdefault((f["QS"], f["KT"], f["HV"], f["TL"]), set()).add(f["DYN_LDS"])
    assert all(len(v) == 1 for v in by_class.values())

"""Child process of tests/test_gpu_pred_forms.py: the two-kernel cases of tests/_pred_cases.py with the fused form switched off
(VBMC_PRED_FUSED=0 is read once per process).  Writes the reported plan and the prediction of every case into one .npz."""
import json
import os
import sys

import numpy as np


def main(out_path):
    assert os.environ.get("VBMC_PRED_FUSED") == "0"
    import vbmc_amd
    from tests import _pred_cases as C
    from vbmc_amd import gplite

    rec = {}
    for name in sorted(n for n, c in C.CASES.items() if c["two_kernel"]):
        d = C.case_inputs(name)      # no reference here: the parent computes it
        rec["plan_" + name] = np.array(json.dumps(gplite.pred_plan(d["gp"], d["Xs"].shape[0])))
        ymu, ys2, fmu, fs2 = vbmc_amd.gplite_pred(d["gp"], d["Xs"], d["ys"], d["s2s"], True)
        rec["ymu_" + name], rec["ys2_" + name], rec["fmu_" + name], rec["fs2_" + name] = ymu, ys2, fmu, fs2
    np.savez(out_path, **rec)
    print("PRED-FORMS-CHILD-OK")


if __name__ == "__main__":
    main(sys.argv[1])

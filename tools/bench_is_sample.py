"""Wall time of the IMIQR importance-sampler set-up (activeimportancesampling_vbmc for acqimiqr_vbmc, profiles/is_sample.md) with its
MCMC driven from the host (device=False: the NumPy ensemble slice sampler, one blocking device prediction per density evaluation) and
run on the device (device=True: vbmc_acq_is_sample), in the same process at the headline GP shape.

Every timing is a host clock around a call that ends synchronised; the median of --reps calls after --warmup calls each.

    python tools/bench_is_sample.py --D 10 --N 400 --S 20 --Nm 100 --thin 1 --reps 10 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--N", type=int, default=400)
    ap.add_argument("--S", type=int, default=20)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--Nm", type=int, default=100)
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from oracle import vbmc_ref as R
    from tests._cases import synth_problem

    p = synth_problem(1, a.D, a.N, a.K, a.S, meanfun=4)
    hyp = p["hyp"].copy()
    hyp[a.D + 1, :] = np.log(0.03)
    gp = R.gplite_post(hyp, p["X"], p["y"], meanfun=4)
    vp = va.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    opts = {"ActiveImportanceSamplingMCMCSamples": a.Nm, "ActiveImportanceSamplingMCMCThin": a.thin}
    eng = va.default_engine()

    def timed(device):
        ts, res = [], None
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            res = va.activeimportancesampling_vbmc(vp, gp, "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(100 + r), engine=eng, device=device)
            eng.ctx.synchronize()
            if r >= a.warmup:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), res

    rows = []
    for device in (False, True):
        med, lo, hi, res = timed(device)
        row = {"path": "device (vbmc_acq_is_sample)" if device else "host-driven (ensemble_slice_sample)", "wall_ms": 1e3 * med, "min_ms": 1e3 * lo,
               "max_ms": 1e3 * hi, "funccount": int(res["funccount"])}
        if device:
            assert "_device" in res, "the device path fell back to the host-driven sampler"
            row.update(rounds=int(res["rounds"]), performed=int(res["performed"]), performed_per_funccount=res["performed"] / res["funccount"])
        rows.append(row)
        print(json.dumps(row))
    out = {"shape": {"D": a.D, "N": a.N, "S": a.S, "Nm": a.Nm, "thin": a.thin, "W": 2 * (a.D + 1)}, "reps": a.reps, "warmup": a.warmup, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

"""Wall time of the IMIQR importance-sampler set-up (activeimportancesampling_vbmc for acqimiqr_vbmc, profiles/is_sample.md) with its
MCMC driven from the host (device=False: the NumPy ensemble slice sampler, one blocking device prediction per density evaluation),
run on the device behind the host's Step 1 (device=True, one_call=False: vbmc_acq_is_sample) and with the whole set-up in one call
(device=True, one_call=True: vbmc_acq_is_setup), in the same process at the headline GP shape.  The second leg is also split by a host
clock around its importance_sample_device call: the front half (Step 1, the resampling, the zero-density check, the upload of x0) is
the call's time less Step 2's.

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

    from vbmc_amd import acq

    step2 = []                                   # host clock inside the second leg: its importance_sample_device call alone
    real_sample = acq.importance_sample_device

    def clocked_sample(*args, **kw):
        eng.ctx.synchronize()
        t0 = time.perf_counter()
        r = real_sample(*args, **kw)
        eng.ctx.synchronize()
        step2.append(time.perf_counter() - t0)
        return r

    acq.importance_sample_device = clocked_sample

    def stats(ts):
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def timed(device, one_call):
        ts, s2, res = [], [], None
        for r in range(a.warmup + a.reps):
            del step2[:]
            t0 = time.perf_counter()
            res = va.activeimportancesampling_vbmc(vp, gp, "acqimiqr_vbmc", None, opts, rng=np.random.default_rng(100 + r), engine=eng, device=device,
                                                   one_call=one_call)
            eng.ctx.synchronize()
            if r >= a.warmup:
                ts.append(time.perf_counter() - t0)
                s2.append(sum(step2))
        return ts, s2, res

    rows = []
    for device, one_call, path in ((False, False, "host-driven (ensemble_slice_sample)"), (True, False, "device Step 2 (vbmc_acq_is_sample)"),
                                   (True, True, "one call (vbmc_acq_is_setup)")):
        ts, s2, res = timed(device, one_call)
        med, lo, hi = stats(ts)
        row = {"path": path, "wall_ms": 1e3 * med, "min_ms": 1e3 * lo, "max_ms": 1e3 * hi, "funccount": int(res["funccount"])}
        if device:
            assert "_device" in res, "the device path fell back to the host-driven sampler"
            row.update(rounds=int(res["rounds"]), performed=int(res["performed"]), performed_per_funccount=res["performed"] / res["funccount"])
        if device and not one_call:
            for name, v in (("step2", s2), ("front", [t - u for t, u in zip(ts, s2)])):
                m_, l_, h_ = stats(v)
                row.update({name + "_ms": 1e3 * m_, name + "_min_ms": 1e3 * l_, name + "_max_ms": 1e3 * h_})
        if one_call:
            assert not step2, "the one-call leg went through vbmc_acq_is_sample (a bad start or a fallback)"
        rows.append(row)
        print(json.dumps(row))
    out = {"shape": {"D": a.D, "N": a.N, "S": a.S, "Nm": a.Nm, "thin": a.thin, "W": 2 * (a.D + 1)}, "reps": a.reps, "warmup": a.warmup, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

"""Wall time of sampling the GP surrogate (gplite_sample, method 'parallel', as gpsample_vbmc calls it: VarThresh = 1;
profiles/gp_surrogate_sample.md) in one device call (vbmc_gp_surrogate_sample) at E = 1, 8 and 32 ensembles against the only way to do
it without that call: the host-driven ``ensemble_slice_sample`` over blocking device ``gplite_pred`` calls, in the same process at the
headline GP shape, from the same high-posterior-density start on the same box.

Every timing is a host clock around a call that ends synchronised; min / median / max of the repetitions after the warm-up calls.

    python tools/bench_gp_surrogate_sample.py --D 10 --N 400 --S 20 --Ns 10000 --reps 5 --host-reps 3 --warmup 1
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
    ap.add_argument("--Ns", type=int, default=10000)
    ap.add_argument("--E", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests._cases import synth_problem
    from vbmc_amd.acq import ensemble_slice_sample
    from vbmc_amd.gplite import _log_gpfun_host, gplite_sample_device

    D, Ns = a.D, a.Ns
    p = synth_problem(1, D, a.N, 2, a.S, meanfun=4)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = np.log(0.03)
    gp = va.gplite_post(hyp, p["X"], p["y"], 1, 4)
    eng = va.default_engine()
    X, y = np.asarray(gp["X"]), np.asarray(gp["y"]).reshape(-1)
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    LB, UB = np.min(X, axis=0) - 10 * diam, np.max(X, axis=0) + 10 * diam      # gplite_sample.m:16-20
    W = 2 * (D + 1)
    hpd = X[np.argsort(-y, kind="stable")[: min(a.N, max(W, int(round(0.25 * a.N))))]]   # :88-101

    def start(E, seed):
        rng = np.random.default_rng(seed)
        return np.stack([hpd[rng.permutation(hpd.shape[0])[:W]] for _ in range(E)])

    VT, burn = 1.0, int(np.ceil(Ns / 5))

    def stats(ts):
        return {"min_ms": 1e3 * float(np.min(ts)), "median_ms": 1e3 * float(np.median(ts)), "max_ms": 1e3 * float(np.max(ts))}

    rows = []
    for E in a.E:
        ts, r = [], None
        for k in range(a.warmup + a.reps):
            x0 = start(E, 100 + k)
            eng.ctx.synchronize()
            t0 = time.perf_counter()
            r = gplite_sample_device(gp, Ns, LB, UB, x0=x0, E=E, VarThresh=VT, seed=1000 + k, outputs=("X",), engine=eng)
            eng.ctx.synchronize()
            if k >= a.warmup:
                ts.append(time.perf_counter() - t0)
        row = dict(path="one device call (vbmc_gp_surrogate_sample)", E=E, **stats(ts), rounds=r["rounds"], funccount=r["funccount"], performed=r["performed"],
                   performed_per_funccount=r["performed"] / r["funccount"], us_per_round=1e6 * float(np.median(ts)) / r["rounds"],
                   mean=np.mean(r["X"], axis=0).tolist())
        rows.append(row)
        print(json.dumps(row))
    if a.host_reps > 0:
        ts, info = [], None
        logp = _log_gpfun_host(gp, 0.0, VT, eng)
        for k in range(a.host_reps):
            x0 = start(1, 100 + k)
            eng.ctx.synchronize()
            t0 = time.perf_counter()
            xs, _, info = ensemble_slice_sample(logp, x0, Ns, LB, UB, thin=1, burnin=burn, rng=np.random.default_rng(1000 + k), return_info=True)
            eng.ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        row = dict(path="host-driven (ensemble_slice_sample over gplite_pred)", E=1, **stats(ts), funccount=info["funccount"], mean=np.mean(xs[0], axis=0).tolist())
        rows.append(row)
        print(json.dumps(row))
        dev1 = next((q for q in rows if q["E"] == 1 and "rounds" in q), None)
        if dev1 is not None:
            print(json.dumps({"acceptance": "device E = 1 slowest repetition < host-driven fastest", "device_max_ms": dev1["max_ms"], "host_min_ms": row["min_ms"],
                              "met": bool(dev1["max_ms"] < row["min_ms"]), "speedup_median": row["median_ms"] / dev1["median_ms"]}))
    out = {"shape": {"D": D, "N": a.N, "S": a.S, "Ns": Ns, "W": W, "VarThresh": VT, "burnin": burn}, "reps": a.reps, "host_reps": a.host_reps, "warmup": a.warmup,
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

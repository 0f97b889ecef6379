"""Wall time of the corner-plot data (vbmc_amd.vptools.vbmc_plot_data -> vbmc_vp_corner; profiles/vp_corner.md) at D = 10, K = 50
(45 pairs) and at D = 32, K = 512 (496 pairs), Ns = 1e5 draws, res = 64, nbins = 40, the median, in one process: cases D and O of
tests/_vptools_ref.py with the component widths doubled (--width).

    the one call        draws, histograms, pair densities and quantiles in one vbmc_vp_corner, copies back included
    the restatement     tests/_corner_ref.corner on the same samples on this machine's host: NumPy / SciPy, NOT MATLAB
                        (--ref-pairs limits it to the first pairs of the larger case and scales; 0: all)

Every timing is a host clock around a call that ends synchronised: median, fastest and slowest of --reps calls after --warmup calls.
--once runs each case once and nothing else: the process to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split.

    python tools/bench_vp_corner.py --reps 10 --warmup 2 --out profiles/vp_corner.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(f, reps, warmup, sync):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "reps": int(reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--Ns", type=int, default=100000)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--width", type=float, default=2.0)
    ap.add_argument("--ref-pairs", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests import _corner_ref as R
    from tests import _vptools_ref as T
    from vbmc_amd import vptools as V

    sync = va.default_engine().ctx.synchronize
    res = {"Ns": a.Ns, "res": a.res, "width": a.width, "rows": []}
    for name in ("D", "O"):
        vp = T.make_case(name, width=a.width)
        call = lambda: V.vbmc_plot_data(vp, a.Ns, seed=1, res=a.res)  # noqa: E731
        dev = call()
        if a.once:
            continue
        D = vp["D"]
        r = {"D": D, "K": vp["K"], "pairs": len(dev["pairs"]), "one_call": clock(call, a.reps, a.warmup, sync)}
        r["no_pairs"] = clock(lambda: V.vbmc_plot_data({**vp, "D": 1, "mu": vp["mu"][:1], "lambda": vp["lambda"][:1], "trinfo": None}, a.Ns, seed=1, res=a.res),
                              a.reps, a.warmup, sync)                     # D = 1: the draw, one histogram, one median, the copies
        npair = len(dev["pairs"]) if a.ref_pairs <= 0 else min(a.ref_pairs, len(dev["pairs"]))
        t0 = time.perf_counter()
        X, b = dev["xx"], dev["bounds"]
        for d in range(D):
            R.hist1(X[:, d], b[d, 0], b[d, 1], 40)
            R.quantile1(X[:, d], 0.5)
        worst = 0.0
        for pp in range(npair):
            d1, d2 = dev["pairs"][pp]
            k = R.kde2d(X[:, [d1, d2]], a.res, b[[d1, d2], 0], b[[d1, d2], 1])
            worst = max(worst, float(np.max(np.abs(k["density"] - dev["density"][pp])) / np.max(k["density"])))
        t = (time.perf_counter() - t0) * 1e3
        r["restatement_ms"], r["restatement_pairs"] = t, npair
        r["restatement_scaled_ms"] = t * len(dev["pairs"]) / npair
        r["density_difference"] = worst
        res["rows"].append(r)
        print(json.dumps(r), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

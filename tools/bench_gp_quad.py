"""Time the Bayesian-quadrature sweep gplite_quad (vbmc_gp_quad) beside the prediction sweep gplite_pred (vbmc_gp_pred) it shares its
kernels with, in one process and interleaved: per hyper-sample outputs at N = 400, D = 10, S = 20, Nstar = 8192 (the search of one
active-sampling step).  Both calls block until their results are on the host.  Writes profiles/gp_quad.md.

    python tools/bench_gp_quad.py [--reps 30] [--quick]
    python tools/bench_gp_quad.py --trace      (a short untimed run to put under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(N, D, S, Nstar, seed=0):
    rng = np.random.default_rng(seed)
    X = 1.5 * rng.standard_normal((N, D))
    y = -0.5 * np.sum(X ** 2, axis=1) + 0.1 * rng.standard_normal(N)
    hyp = np.zeros((3 * D + 3, S))
    hyp[:D] = np.log(0.8) + 0.2 * rng.standard_normal((D, S))
    hyp[D] = np.log(np.std(y)) + 0.1 * rng.standard_normal(S)
    hyp[D + 1] = np.log(0.03)
    hyp[D + 2] = np.max(y)
    hyp[D + 3:2 * D + 3] = 0.2 * rng.standard_normal((D, S))
    hyp[2 * D + 3:] = np.log(2.0) + 0.1 * rng.standard_normal((D, S))
    Xs = 1.3 * rng.standard_normal((Nstar, D))
    delta = 0.05 + 0.2 * rng.random(D)
    return hyp, X, y, Xs, delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_quad.md"))
    a = ap.parse_args()
    import vbmc_amd as va

    N, D, S, Nstar = (100, 4, 3, 512) if a.quick else (400, 10, 20, 8192)
    hyp, X, y, Xs, delta = problem(N, D, S, Nstar)
    gp = va.gplite_post(hyp, X, y, 1, 4, need_L=False)
    calls = {"gplite_pred": lambda: va.gplite_pred(gp, Xs, None, None, True), "gplite_quad": lambda: va.gplite_quad(gp, Xs, delta, True)}
    for _ in range(3):                                  # warm-up: code objects, inv(L') of the GP, the pooled buffers
        for f in calls.values():
            f()
    if a.trace:
        for _ in range(5):
            for f in calls.values():
                f()
        return
    ts = {k: [] for k in calls}
    for _ in range(a.reps):                             # interleaved: drift of the clocks hits both alike
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()                                         # returns with the results on the host: the device is idle again
            ts[k].append(1e3 * (time.perf_counter() - t0))
    row = {"N": N, "D": D, "S": S, "Nstar": Nstar, "reps": a.reps}
    for k, v in ts.items():
        v = np.sort(v)
        row[k] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v[0]), 3), "p10_ms": round(float(v[len(v) // 10]), 3),
                  "p90_ms": round(float(v[(9 * len(v)) // 10]), 3)}
    row["quad_over_pred_median"] = round(row["gplite_quad"]["median_ms"] / row["gplite_pred"]["median_ms"], 4)
    print(json.dumps(row))
    keep = ""                                           # the hand-written part of the file, from its "## Reading" heading on, survives a re-run
    if os.path.exists(a.out):
        txt = open(a.out).read()
        if "\n## Reading" in txt:
            keep = txt[txt.index("\n## Reading"):]
    with open(a.out, "w") as f:
        f.write("# vbmc_gp_quad beside vbmc_gp_pred: the acquisition sweep's mean and variance with and without vp.delta\n\n")
        f.write("`python tools/bench_gp_quad.py --reps %d%s`: N = %d, D = %d, S = %d, Nstar = %d, meanfun 4, per hyper-sample outputs; wall time of "
                "the blocking call (upload of the points, kernels, readback), %d calls each, interleaved, after three warm-up calls.\n\n"
                % (a.reps, " --quick" if a.quick else "", N, D, S, Nstar, a.reps))
        f.write("| call | median, ms | min | 10th - 90th percentile |\n|---|---|---|---|\n")
        for k in calls:
            r = row[k]
            f.write("| `%s` | %.3f | %.3f | %.3f - %.3f |\n" % (k, r["median_ms"], r["min_ms"], r["p10_ms"], r["p90_ms"]))
        f.write("\nquadrature / prediction (medians): %.4f\n\n```\n%s\n```\n%s" % (row["quad_over_pred_median"], json.dumps(row), keep))


if __name__ == "__main__":
    main()

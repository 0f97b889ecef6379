"""Time the device-resident optimisation half of gplite_train (vbmc_gp_train_optimize) against the path it replaces: the fill
stage as one batched gplite_nlZ call and scipy's L-BFGS-B over blocking gplite_nlZ calls from the same starts.  Writes
profiles/gp_train_optimize.md.

    python tools/bench_gp_train.py [--reps 5] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(N, D, seed=0):
    rng = np.random.default_rng(seed)
    sd = np.arange(1, D + 1, dtype=np.float64)
    X = np.concatenate([rng.standard_normal((3 * N // 4, D)) * 1.2 * sd, rng.uniform(-2 * D, 2 * D, size=(N - 3 * N // 4, D))], axis=0)
    y = np.sum(-0.5 * (X / sd) ** 2, axis=1) + 0.01 * rng.standard_normal(N)
    h0 = np.concatenate([np.log(np.std(X, axis=0)), [np.log(np.std(y))], [np.log(1e-2)], [np.max(y)], np.mean(X, axis=0), np.log(np.std(X, axis=0))])
    lb = np.concatenate([h0[:D] - 4, [h0[D] - 6], [np.log(1e-4)], [np.max(y) - 10 * np.ptp(y)], np.min(X, axis=0), h0[D + 3 + D:] - 3])
    ub = np.concatenate([h0[:D] + 4, [h0[D] + 6], [np.log(2.0)], [np.max(y) + 10 * np.ptp(y)], np.max(X, axis=0), h0[D + 3 + D:] + 3])
    gp = {"X": X, "y": y, "s2": None, "covfun": 1, "Ncov": D + 1, "noisefun": (1, 0, 0), "Nnoise": 1, "meanfun": 4, "Nmean": 2 * D + 1, "intmeanfun": 0}
    return gp, h0, lb, ub, h0 - 0.25 * (h0 - lb), h0 + 0.25 * (ub - h0)


def host_path(va, gp, design, starts, lb, ub, tol):
    """What a caller had before: the fill as ONE batched gplite_nlZ call, then L-BFGS-B over blocking calls from the same starts."""
    from scipy.optimize import minimize

    t0 = time.perf_counter()
    va.gplite_nlZ(design.T.copy(), gp, None, 1)
    t_fill = time.perf_counter() - t0
    evals = [0]

    def f(h):
        evals[0] += 1
        nlz, g = va.gplite_nlZ(h, gp, None, 2)
        return float(nlz), np.asarray(g, dtype=np.float64).reshape(-1)

    t0 = time.perf_counter()
    funs = [minimize(f, s, jac=True, method="L-BFGS-B", bounds=list(zip(lb, ub)), options={"maxiter": 1000, "ftol": tol, "gtol": tol}).fun for s in starts.T]
    return t_fill, time.perf_counter() - t0, evals[0], funs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_train_optimize.md"))
    a = ap.parse_args()
    import vbmc_amd as va

    N, D, tol = (100, 4, 1e-5) if a.quick else (400, 10, 1e-5)
    gp, h0, lb, ub, plb, pub = problem(N, D)
    rows, lines = [], []
    for Ninit, Nopts in ((1024, 2), (64, 1)):
        design = va.fminfill_design(h0[None], lb, ub, plb, pub, None, Ninit, seed=1)
        res = {}
        for W in (1, 2, 4):
            ts = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                out = va.gplite_train_optimize(gp, h0, lb, ub, plb, pub, None, {"Design": design, "Nopts": Nopts, "TolFun": tol, "W": W})
                ts.append(time.perf_counter() - t0)
            res[W] = (sorted(ts[1:]), out)
        out1 = res[1][1]
        # the same starts for the host path: the device's own (sorted fill, low-noise pick, clamp)
        o0 = va.gplite_train_optimize(gp, h0, lb, ub, plb, pub, None, {"Design": design, "Nopts": Nopts, "TolFun": tol, "MaxIter": 1, "MaxFunEvals": 1})
        hp = [host_path(va, gp, design, o0["hyp"], lb, ub, tol) for _ in range(min(a.reps, 3))]
        t_fill, t_opt, n_ev, funs = sorted(hp, key=lambda r: r[0] + r[1])[len(hp) // 2]
        fc = int(np.sum(out1["funccount"]))
        row = {"N": N, "D": D, "Ninit": Ninit, "Nopts": Nopts, "device_ms": {W: [round(1e3 * t, 2) for t in res[W][0]] for W in res},
               "device_funccount": fc, "device_performed": {W: res[W][1]["performed"] for W in res}, "device_nll": [float(v) for v in out1["nll"]],
               "device_exitflag": [int(v) for v in out1["exitflag"]], "device_iterations": [int(v) for v in out1["iterations"]],
               "host_fill_ms": round(1e3 * t_fill, 2), "host_opt_ms": round(1e3 * t_opt, 2), "host_evals": n_ev, "host_nll": [float(v) for v in funs]}
        rows.append(row)
        med = {W: float(np.median(res[W][0])) for W in res}
        lines.append("| %d | %d | %s | %d | %.3f | %.1f + %.1f | %d | %.3f | %s | %s |" % (
            Ninit, Nopts, " / ".join("%.1f" % (1e3 * med[W]) for W in (1, 2, 4)), fc, 1e3 * med[1] / (Ninit + fc), 1e3 * t_fill, 1e3 * t_opt, n_ev,
            1e3 * t_opt / max(n_ev, 1), " ".join("%.4f" % v for v in out1["nll"]), " ".join("%.4f" % v for v in funs)))
        print(json.dumps(row))
    keep = ""                                    # the hand-written part of the file, from its "## Reading" heading on, survives a re-run
    if os.path.exists(a.out):
        txt = open(a.out).read()
        if "\n## Reading" in txt:
            keep = txt[txt.index("\n## Reading"):]
    with open(a.out, "w") as f:
        f.write("# vbmc_gp_train_optimize: the optimisation half of gplite_train on the device\n\n")
        f.write("`python tools/bench_gp_train.py --reps %d%s`: N = %d, D = %d, meanfun 4, TolFun %g; wall time of the whole call "
                "(upload, fill, starts, optimiser, results), median of %d runs after one warm-up.\n\n" % (a.reps, " --quick" if a.quick else "", N, D, tol, a.reps))
        f.write("| Ninit | Nopts | device call, ms (W = 1 / 2 / 4) | optimiser evaluations | ms per evaluation (fill + optimiser, W = 1) | "
                "host path: batched fill + L-BFGS-B over blocking calls, ms | its evaluations | ms per blocking evaluation | device nll | host nll |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n" + keep)


if __name__ == "__main__":
    main()

"""Wall time of one gplite_train-style slice-sampling chain of GP hyper-parameters (profiles/gp_slice_sample.md).

Baseline: the host-driven chain -- the one-evaluation-at-a-time loop of slicesamplebnd (tests/_slice_ref.py) calling
vbmc_amd.gplite_nlZ once per evaluation plus the host hyper-prior, which is how such a chain had to be run before
vbmc_gp_slice_sample existed.  Device chain: vbmc_amd.slicesamplebnd_gp at the speculation widths asked for, same uniform block.
Every timing is a host clock around a call that ends synchronised; the median of --reps runs after one warm-up run each.

    python tools/bench_gp_sample.py --N 400 --D 10 --Ns 20 --thin 5 --burnin 100 --W 1 2 4 8 16 --reps 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_problem(N, D, meanfun, seed):
    rng = np.random.default_rng(seed)
    X = 1.5 * rng.standard_normal((N, D))
    y = -0.5 * np.sum((X / 1.3) ** 2, axis=1) + 0.3 * np.sin(X[:, 0]) + 0.05 * rng.standard_normal(N)
    Nmean = {0: 0, 1: 1, 4: 2 * D + 1}[meanfun]
    gp = {"X": X, "y": y, "s2": None, "covfun": 1, "Ncov": D + 1, "noisefun": (1, 0, 0), "Nnoise": 1, "meanfun": meanfun, "Nmean": Nmean,
          "meanfun_extras": None, "intmeanfun": 0}
    h = np.zeros(D + 2 + Nmean)
    h[:D] = np.log(0.8)
    h[D] = np.log(np.std(y))
    h[D + 1] = np.log(5e-2)
    if meanfun >= 1:
        h[D + 2] = np.max(y)
    if meanfun == 4:
        h[D + 3 + D:] = np.log(2.0)
    Nhyp = h.size
    hp = {"mu": h.copy(), "sigma": 2.0 * np.ones(Nhyp), "df": 3.0 * np.ones(Nhyp)}
    return gp, hp, h, h - 5.0, h + 5.0, 0.5 * np.ones(Nhyp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=400)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--meanfun", type=int, default=4)
    ap.add_argument("--Ns", type=int, default=20)
    ap.add_argument("--thin", type=int, default=5)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--W", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kmax", type=int, default=60)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests._slice_ref import make_block, slicesamplebnd

    gp, hp, x0, LB, UB, widths = make_problem(a.N, a.D, a.meanfun, 1)
    Neff = a.Ns * a.thin                           # gplite_train.m:314: Ns * Thin sweeps recorded, thinned afterwards
    opts = {"Thin": 1, "Burnin": a.burnin}
    perms, U = make_block(np.random.default_rng(2), Neff + a.burnin, x0.size, a.kmax)
    eng = va.default_engine()

    def timed(fn):
        fn()                                        # warm-up: code objects, pool blocks, pinned memory
        ts, res = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = fn()
            eng.ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), res

    rows = []
    base = None
    if not a.no_baseline:
        logf = lambda x: -(va.gplite_nlZ(x, gp, None, nargout=1) - va.gplite_hypprior(x, hp, nargout=1))  # noqa: E731
        med, lo, hi, (bs, bf, bo) = timed(lambda: slicesamplebnd(logf, x0, Neff, widths, LB, UB, opts, perms, U))
        base = (bs, bf, bo)
        rows.append({"chain": "host loop + vbmc_gp_nlz (B = 1)", "W": None, "wall_s": med, "min_s": lo, "max_s": hi, "sequential_evals": bo["funccount"],
                     "performed": bo["funccount"], "us_per_sequential_eval": 1e6 * med / bo["funccount"], "maxshrink": bo["maxshrink"]})
    first = None
    for W in a.W:
        med, lo, hi, (s, f, _, out) = timed(lambda: va.slicesamplebnd_gp(gp, hp, x0, Neff, widths, LB, UB, opts, uniforms=U, perms=perms, W=W))
        if first is None:
            first = (s, f, out)
        same = bool(np.array_equal(s, first[0]) and np.array_equal(f, first[1]) and out.funccount == first[2].funccount)
        row = {"chain": "device chain", "W": W, "wall_s": med, "min_s": lo, "max_s": hi, "sequential_evals": out.funccount, "performed": out.performed,
               "us_per_sequential_eval": 1e6 * med / out.funccount, "maxshrink": out.maxshrink, "bit_identical_to_first_W": same,
               "rounds_done": out.rounds_done, "rounds_enqueued": out.rounds_enqueued}
        if base is not None:
            row["max_abs_diff_samples_vs_host_loop"] = float(np.max(np.abs(s - base[0])))
            row["same_sequential_evals_as_host_loop"] = bool(out.funccount == base[2]["funccount"])
        rows.append(row)
    res = {"shape": {"N": a.N, "D": a.D, "meanfun": a.meanfun, "Nhyp": int(x0.size), "Ns": a.Ns, "Thin": a.thin, "Burnin": a.burnin,
                     "sweeps": Neff + a.burnin}, "reps": a.reps, "rows": rows}
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

"""Wall time of the mode of the variational posterior (vbmc_amd.vptools.vbmc_mode -> vbmc_vp_mode; profiles/vp_mode.md) at D = 10,
K = 50 (transform types alternating 0 / 3) and at D = 32, K = 512 (types 3 / 0 with scale and rotation), nmax = 20, both flags, in
one process.  The posteriors are cases D and O of tests/_vptools_ref.py with the component widths doubled (--width), so that
neighbouring components overlap and a start is not already a maximum:

    the one call            ranking, every start's BFGS and the way back in one vbmc_vp_mode
    the host-driven loop    the same BFGS (tests/_mode_ref.bfgs's rules) driven from the host with one blocking vbmc_vp_pdf(..., dy)
                            per objective evaluation; origflag = 0 only, since the pdf entry point refuses the original-space gradient

Every timing is a host clock around a call that ends synchronised: median, fastest and slowest of --reps calls after --warmup calls.
The per-iteration time is the one call's median over the largest iteration count among its starts (the workgroups run side by side, so
the slowest start sets the call's length), launch and copies included.

    python tools/bench_vp_mode.py --reps 20 --warmup 3 --out profiles/vp_mode.json --md profiles/vp_mode.md
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


def host_driven(V, M, vp, nmax):
    """The library's optimiser with every objective evaluation a blocking device call; returns (x, fs, evaluations, iterations)"""
    D, K, mu, sigma, lam, w = M._parts(vp)
    evals = [0]

    def fg(u):
        evals[0] += 1
        y, dy = V.vbmc_pdf(vp, u[None, :], False, True, nargout=2)
        return -float(y[0]), -dy[0]

    if nmax < K:
        f_all = V.vbmc_pdf(vp, mu, False, True)
        comps = np.argsort(-f_all, kind="stable")[:nmax]
    else:
        comps = np.arange(K)
    us, fs, iters = [], [], 0
    for c in comps:
        u, H = mu[c].copy(), np.diag((sigma[c] * lam) ** 2)
        f, g = fg(u)
        for _ in range(M.MAX_ITER):
            if np.max(np.abs(g)) <= M.TOL_GRAD:
                break
            d = -H @ g
            gd, take = g @ d, None
            for k in range(M.KMAX):
                t = 2.0 ** -k
                fc, gc = fg(u + t * d)
                if fc <= f + M.C1 * t * gd:
                    take = (u + t * d, fc, gc)
                    break
            if take is None:
                break
            s, y = take[0] - u, take[2] - g
            ys, Hy = y @ s, H @ y
            if ys > 0 and ys * ys > M.CURV ** 2 * (s @ s) * (y @ y):
                rho = 1.0 / ys
                H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + rho * (1 + rho * (y @ Hy)) * np.outer(s, s)
            u, f, g = take
            iters += 1
        us.append(u)
        fs.append(-f)
    return us[int(np.argmax(fs))], np.array(fs), evals[0], iters


def fmt(t):
    return "%.3f | %.3f | %.3f | %d" % (t["median_ms"], t["min_ms"], t["max_ms"], t["reps"])


def write_md(res, path):
    L = ["# The mode of the variational posterior in one call (`vbmc_vp_mode`)", "",
         "Written by `tools/bench_vp_mode.py` on one MI355X; every number is of that run.  nmax = %d starts.  Host clock around calls that "
         "end synchronised; ms.  Cases D and O of `tests/_vptools_ref.py`, component widths times %g." % (res["nmax"], res["width"]), "",
         "| D | K | origflag | leg | median | fastest | slowest | calls | largest iteration count of a start | objective evaluations | per iteration (µs) |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        L.append("| %d | %d | %d | one call | %s | %d | %d (device, all starts) | %s |" % (
            r["D"], r["K"], r["origflag"], fmt(r["one_call"]), r["iters_max"], r["nfev_sum"], "%.1f" % r["us_per_iter"] if r["iters_max"] else "-"))
        if "host_loop" in r:
            L.append("| %d | %d | %d | host-driven BFGS, one blocking `vbmc_vp_pdf(..., dy)` per evaluation | %s | | %d | %.1f per evaluation |" % (
                r["D"], r["K"], r["origflag"], fmt(r["host_loop"]), r["host_evals"], 1e3 * r["host_loop"]["median_ms"] / max(r["host_evals"], 1)))
    L += ["", "Ratio of the host-driven loop to the one call (medians): " + "; ".join(
        "D = %d, K = %d: %.1f (largest |x_host - x_device| %.2e)" % (r["D"], r["K"], r["ratio"], r["x_difference"]) for r in res["rows"] if "ratio" in r) + ".", "",
        "The host-driven loop evaluates one candidate of the line search at a time and stops at the first acceptable one; the device "
        "evaluates four at a time, so its evaluation count is the larger for the same iterations.", ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--nmax", type=int, default=20)
    ap.add_argument("--width", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests import _mode_ref as M
    from tests import _vptools_ref as T
    from vbmc_amd import vptools as V

    sync = va.default_engine().ctx.synchronize
    res = {"nmax": a.nmax, "width": a.width, "rows": []}
    for name in ("D", "O"):
        vp = T.make_case(name, width=a.width)
        for origflag in (0, 1):
            x, det = V.vbmc_mode(vp, a.nmax, origflag, details=True)
            r = {"D": vp["D"], "K": vp["K"], "origflag": origflag, "iters_max": int(det["iters"].max()), "nfev_sum": int(det["nfev"].sum()),
                 "stops": np.bincount(det["stop"], minlength=4)[1:].tolist()}
            r["one_call"] = clock(lambda: V.vbmc_mode(vp, a.nmax, origflag), a.reps, a.warmup, sync)
            r["us_per_iter"] = 1e3 * r["one_call"]["median_ms"] / max(r["iters_max"], 1)
            if not origflag:
                xh, fsh, ev, it = host_driven(V, M, vp, a.nmax)
                r["host_loop"] = clock(lambda: host_driven(V, M, vp, a.nmax), a.host_reps, 1, sync)
                r["host_evals"], r["host_iters"] = int(ev), int(it)
                r["ratio"] = r["host_loop"]["median_ms"] / r["one_call"]["median_ms"]
                r["x_difference"] = float(np.max(np.abs(xh - x)))
            res["rows"].append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        write_md(res, a.md)


if __name__ == "__main__":
    main()

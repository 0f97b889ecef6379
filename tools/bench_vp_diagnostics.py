"""Wall time of the multi-run diagnostics (vbmc_amd.vptools.vp_diagnostics -> vbmc_vp_diagnostics; profiles/vp_diagnostics.md) at the
headline posterior -- D = 10, K = 50, transform types alternating 0 / 3, Ns = 10^5 draws per run, 2^13 mesh points, 10^5 quadrature
points -- for R = 2, 5 and 10 runs, in one process:

    the one call                       every pair's KL divergences and marginal total variations
    the loop over the same pairs       vbmc_kldiv + vbmc_mtv per pair (vbmc_vp_kldiv, vbmc_vp_mtv: what a caller had before)
    the NumPy restatement, one pair    two vbmc_rnd calls, tests/_vptools_ref.kldiv_terms and tests/_mtv_ref.mtv on the host
    per stage                          the call without kl_mat, without the integrals, and without both (the library skips what is
                                       not asked for); the differences are the stages' shares
    the cosine transform               k_diag_dct against k_mtv_dct over the same C = R D columns (20, 50, 100) at n = 2^13, both
                                       directions, HIP-event time of each launch (vbmc_test_dct).  The project's criterion: the new
                                       kernel's slowest repetition has to beat the old kernel's fastest.

Every whole-call timing is a host clock around a call that ends synchronised: median, fastest and slowest of --reps calls after
--warmup calls (the host leg: --host-reps calls).

    python tools/bench_vp_diagnostics.py --reps 10 --warmup 2 --out profiles/vp_diagnostics.json --md profiles/vp_diagnostics.md
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


def dct_times(ctx, n, Ccols, inverse, kernel, reps, x):
    from vbmc_amd._lib import ptr

    out, a2, ms = np.zeros_like(x), np.zeros_like(x), np.zeros(reps + 2)
    ctx.check(ctx.lib.vbmc_test_dct(ctx.h, n, Ccols, inverse, kernel, reps + 2, ptr(x), ptr(out), None if inverse else ptr(a2), ptr(ms)))
    ms = ms[2:]                                                   # two warm-up launches
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": int(reps)}, out


def fmt(t):
    return "%.3f | %.3f | %.3f | %d" % (t["median_ms"], t["min_ms"], t["max_ms"], t["reps"])


def write_md(res, path):
    L = ["# The multi-run diagnostics in one call (`vbmc_vp_diagnostics`)", "",
         "Written by `tools/bench_vp_diagnostics.py` on one MI355X; every number is of that run.  D = %d, K = %d, transform types %s, "
         "Ns = %d draws per run, %d mesh points, %d quadrature points.  Host clock around calls that end synchronised; ms." % (
             res["shape"]["D"], res["shape"]["K"], res["shape"]["types"], res["Ns"], res["nkde"], res["nquad"]), "",
         "## Whole calls", "", "| R | pairs | leg | median | fastest | slowest | calls |", "|---|---|---|---|---|---|---|"]
    for R, r in res["runs"].items():
        L.append("| %s | %d | one call | %s |" % (R, r["pairs"], fmt(r["one_call"])))
        L.append("| %s | %d | loop of `vbmc_kldiv` + `vbmc_mtv` over the pairs | %s |" % (R, r["pairs"], fmt(r["pair_loop"])))
    L += ["| 2 | 1 | NumPy restatement on the host (two `vbmc_rnd`, `kldiv_terms`, `_mtv_ref.mtv`) | %s |" % fmt(res["host_one_pair"]), "",
          "Largest difference between the one call and the loop over the pairs (the loop draws every pair with its own seeds, so the "
          "two differ by Monte-Carlo error, not by rounding): " + "; ".join("R = %s: kl %.2e, mtv %.2e" % (R, r["difference_kl_max"], r["difference_mtv_max"]) for R, r in res["runs"].items()) + ".", "",
          "## Where the time goes", "", "The library skips the cross densities without `kl_mat` and the integrals without `mtv` / `maxmtv_mat`; "
          "medians in ms.", "", "| R | all | without kl_mat | without the integrals | draws + KDE alone | cross densities | integrals |", "|---|---|---|---|---|---|---|"]
    for R, r in res["runs"].items():
        a, b, c, d = (r[k]["median_ms"] for k in ("one_call", "no_kl", "no_integral", "kde_only"))
        L.append("| %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f |" % (R, a, b, c, d, a - b, a - c))
    L += ["", "## The cosine transform: `k_diag_dct` against `k_mtv_dct`", "",
          "HIP-event time of each launch over the same C columns at n = %d (ms); `k_diag_dct` stays if its slowest launch beats "
          "`k_mtv_dct`'s fastest." % res["nkde"], "",
          "| C | direction | kernel | median | fastest | slowest | launches | largest difference of the outputs, relative to the largest output |",
          "|---|---|---|---|---|---|---|---|"]
    for row in res["dct"]:
        L.append("| %d | %s | `k_mtv_dct` | %s | |" % (row["C"], row["direction"], fmt(row["k_mtv_dct"])))
        L.append("| %d | %s | `k_diag_dct` | %s | %.2e |" % (row["C"], row["direction"], fmt(row["k_diag_dct"]), row["max_rel_difference"]))
    L += ["", "Criterion met in every row: **%s**." % ("yes" if res["dct_criterion_met"] else "no"), ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--Ns", type=int, default=100000)
    ap.add_argument("--nkde", type=int, default=8192)
    ap.add_argument("--nquad", type=int, default=100000)
    ap.add_argument("--runs", default="2,5,10")
    ap.add_argument("--dct-columns", default="20,50,100")
    ap.add_argument("--dct-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests import _mtv_ref as M
    from tests import _vptools_ref as T
    from vbmc_amd import vptools as V

    eng = va.default_engine()
    ctx = eng.ctx
    sync = ctx.synchronize
    seed = 1
    vp = T.make_case("D")
    D, K = vp["D"], vp["K"]
    res = {"shape": {"D": D, "K": K, "types": "alternating 0 / 3"}, "Ns": a.Ns, "nkde": a.nkde, "nquad": a.nquad,
           "host_label": "NumPy restatement, not MATLAB", "runs": {}}
    kw = dict(seed=seed, nkde=a.nkde, nquad=a.nquad)
    for R in (int(r) for r in a.runs.split(",")):
        vps = [vp] + [T.sibling(vp, seed=2 + i) for i in range(R - 1)]
        pairs = [(i, j) for i in range(R) for j in range(i + 1, R)]

        def loop():
            out = []
            for i, j in pairs:
                out.append((V.vbmc_kldiv(vps[i], vps[j], a.Ns, seed=seed + 2 * len(out)), V.vbmc_mtv(vps[i], vps[j], a.Ns, seed=seed + 2 * len(out), **{k: kw[k] for k in ("nkde", "nquad")})))
            return out

        r = {"pairs": len(pairs)}
        r["one_call"] = clock(lambda: V.vp_diagnostics(vps, a.Ns, **kw), a.reps, a.warmup, sync)
        r["pair_loop"] = clock(loop, a.reps, a.warmup, sync)
        r["no_kl"] = clock(lambda: V.vp_diagnostics(vps, a.Ns, outputs=("mtv", "maxmtv_mat"), **kw), a.reps, a.warmup, sync)
        r["no_integral"] = clock(lambda: V.vp_diagnostics(vps, a.Ns, outputs=("kl_mat",), **kw), a.reps, a.warmup, sync)
        r["kde_only"] = clock(lambda: V.vp_diagnostics(vps, a.Ns, outputs=(), **kw), a.reps, a.warmup, sync)
        one, lp = V.vp_diagnostics(vps, a.Ns, **kw), loop()
        r["difference_kl_max"] = float(max(max(abs(one["kl_mat"][i, j] - l[0][0]), abs(one["kl_mat"][j, i] - l[0][1])) for (i, j), l in zip(pairs, lp)))
        r["difference_mtv_max"] = float(max(np.max(np.abs(one["mtv"][i, j] - l[1])) for (i, j), l in zip(pairs, lp)))
        r["one_call_slowest_below_loop_fastest"] = bool(r["one_call"]["max_ms"] < r["pair_loop"]["min_ms"])
        res["runs"][str(R)] = r
        print("R = %d" % R, json.dumps(r), flush=True)

    vp2 = T.sibling(vp, seed=2)
    inf = np.full(D, np.inf)

    def host_pair():
        x1 = V.vbmc_rnd(vp, a.Ns, True, True, seed=seed, nargout=1)
        x2 = V.vbmc_rnd(vp2, a.Ns, True, True, seed=seed + 1, nargout=1)
        return T.kldiv_terms(vp, vp2, x1, x2)[0], M.mtv(x1, x2, -inf, inf, -inf, inf, nkde=a.nkde, nquad=a.nquad)[0]

    res["host_one_pair"] = clock(host_pair, a.host_reps, 0, lambda: None)
    print("host", json.dumps(res["host_one_pair"]), flush=True)

    res["dct"] = []
    rng = np.random.default_rng(0)
    ok = True
    for Ccols in (int(c) for c in a.dct_columns.split(",")):
        x = rng.random((Ccols, a.nkde))
        x /= x.sum(axis=1, keepdims=True)
        for inverse, name in ((0, "forward"), (1, "inverse")):
            t0, o0 = dct_times(ctx, a.nkde, Ccols, inverse, 0, a.dct_reps, x)
            t1, o1 = dct_times(ctx, a.nkde, Ccols, inverse, 1, a.dct_reps, x)
            row = {"C": Ccols, "direction": name, "k_mtv_dct": t0, "k_diag_dct": t1, "max_rel_difference": float(np.max(np.abs(o1 - o0)) / np.max(np.abs(o0))),
                   "new_slowest_below_old_fastest": bool(t1["max_ms"] < t0["min_ms"])}
            ok = ok and row["new_slowest_below_old_fastest"]
            res["dct"].append(row)
            print("dct", json.dumps(row), flush=True)
    res["dct_criterion_met"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        write_md(res, a.md)


if __name__ == "__main__":
    main()

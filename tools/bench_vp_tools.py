"""Wall time of the variational-posterior tools (vbmc_amd.vptools, profiles/vp_tools.md) at the headline posterior -- D = 10, K = 50,
transform types alternating 0 / 3 -- in one process:

    vbmc_pdf      10^6 points     against the NumPy restatement on this box's host
    vbmc_rnd      3 10^5 draws    (with the copy to the host) against the restatement
    vbmc_moments  10^6 draws      against the restatement and against this library's own vbmc_rnd + host cov
    vbmc_kldiv    10^5 draws      against the restatement and against this library's own vbmc_rnd + vbmc_pdf
    vbmc_mtv      10^5 draws      the whole device call against two vbmc_rnd calls + the NumPy restatement (tests/_mtv_ref.py) on the host
    transformed-space pdf / rnd   against the host forms the package had before (acq._vbmc_lnpdf, acq.vbmc_rnd)

The host legs are the NumPy restatement (tests/_vptools_ref.py), not MATLAB.  Every timing is a host clock around a call that ends
synchronised: median, fastest and slowest of --reps calls after --warmup calls (the host legs: --host-reps calls).  For k_vp_pdf the
point-component pairs per second and the fraction of the fp64 pipe by the accounting of SURVEY.md section 8d are reported too.

    python tools/bench_vp_tools.py --reps 10 --warmup 2 --out profiles/vp_tools.json
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
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--Npdf", type=int, default=1000000)
    ap.add_argument("--Nrnd", type=int, default=300000)
    ap.add_argument("--Nmom", type=int, default=1000000)
    ap.add_argument("--Nkl", type=int, default=100000)
    ap.add_argument("--Nmtv", type=int, default=100000)
    ap.add_argument("--only-mtv", action="store_true", help="the vbmc_mtv leg alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import vbmc_amd as va
    from tests import _vptools_ref as T
    from vbmc_amd import acq
    from vbmc_amd import vptools as V

    eng = va.default_engine()
    sync = eng.ctx.synchronize
    nosync = lambda: None
    vp = T.make_case("D")
    vp2 = T.sibling(vp, 2)
    D, K = vp["D"], vp["K"]
    res = {"shape": {"D": D, "K": K, "types": "alternating 0 / 3"}, "host_label": "NumPy restatement, not MATLAB"}
    seed = 1

    def composed_mtv():
        from tests import _mtv_ref as M

        x1 = V.vbmc_rnd(vp, a.Nmtv, True, True, seed=seed, nargout=1)
        x2 = V.vbmc_rnd(vp2, a.Nmtv, True, True, seed=seed + 1, nargout=1)
        return M.mtv(x1, x2, *M.bounds_of(vp, D), *M.bounds_of(vp2, D))[0]

    res["mtv_device"] = clock(lambda: V.vbmc_mtv(vp, vp2, a.Nmtv, seed=seed), a.reps, a.warmup, sync)
    res["mtv_rnd_plus_host_restatement"] = clock(composed_mtv, a.host_reps, 0, nosync)
    res["mtv_max_abs_difference"] = float(np.max(np.abs(V.vbmc_mtv(vp, vp2, a.Nmtv, seed=seed) - composed_mtv())))
    if a.only_mtv:
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return

    X = V.vbmc_rnd(vp, a.Npdf, True, True, seed=seed, nargout=1)
    Y = V.vbmc_rnd(vp, a.Npdf, False, True, seed=seed, nargout=1)
    res["pdf_device"] = clock(lambda: V.vbmc_pdf(vp, X, True, True), a.reps, a.warmup, sync)
    res["pdf_host"] = clock(lambda: T.pdf(vp, X, True, True), a.host_reps, 0, nosync)
    res["pdf_trans_device"] = clock(lambda: V.vbmc_pdf(vp, Y, False, True), a.reps, a.warmup, sync)
    res["pdf_trans_parent_host"] = clock(lambda: acq._vbmc_lnpdf(vp, Y[:100000]), a.host_reps, 0, nosync)
    res["pdf_trans_parent_host"]["points"] = 100000          # (N x K x D temporaries: a tenth of the points, scaled below)
    pairs = a.Npdf * K
    t = res["pdf_device"]["median_ms"] * 1e-3
    # SURVEY 8d's accounting: fp64 VALU operations per pair over the pipe's rate (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz, one per lane and clock)
    DT = 12
    ops_pair = 2 * DT + 2 + 17           # sub + fma per padded dimension, the argument, the table exponential and the running sum
    res["pdf_pairs_per_s"] = pairs / t
    res["pdf_fp64_pipe_fraction_whole_call"] = pairs * ops_pair / t / (256 * 4 * 16 * 2.4e9)

    B, _ = V.vp_rnd_rng_dump(seed, a.Nrnd, D, vp["w"], True)
    res["rnd_device"] = clock(lambda: V.vbmc_rnd(vp, a.Nrnd, True, True, seed=seed), a.reps, a.warmup, sync)
    res["rnd_host_given_the_block"] = clock(lambda: T.rnd(vp, a.Nrnd, True, True, B, seed), a.host_reps, 0, nosync)
    res["rnd_trans_device"] = clock(lambda: V.vbmc_rnd(vp, a.Nrnd, False, True, seed=seed), a.reps, a.warmup, sync)
    rng = np.random.default_rng(0)
    res["rnd_trans_parent_host"] = clock(lambda: acq.vbmc_rnd(vp, a.Nrnd, False, True, rng=rng), a.host_reps, 0, nosync)

    res["moments_fused"] = clock(lambda: V.vbmc_moments(vp, True, a.Nmom, seed=seed), a.reps, a.warmup, sync)
    res["moments_composed"] = clock(lambda: T.moments(V.vbmc_rnd(vp, a.Nmom, True, True, seed=seed, nargout=1)), a.reps, a.warmup, sync)
    Bm, _ = V.vp_rnd_rng_dump(seed, a.Nmom, D, vp["w"], True)
    res["moments_host_given_the_block"] = clock(lambda: T.moments(T.rnd(vp, a.Nmom, True, True, Bm, seed)[0]), a.host_reps, 0, nosync)

    def composed_kl():
        x1 = V.vbmc_rnd(vp, a.Nkl, True, True, seed=seed, nargout=1)
        x2 = V.vbmc_rnd(vp2, a.Nkl, True, True, seed=seed + 1, nargout=1)
        q = [V.vbmc_pdf(p, x, True) for p, x in ((vp, x1), (vp2, x1), (vp, x2), (vp2, x2))]
        return -np.mean(np.log(q[1]) - np.log(q[0])), -np.mean(np.log(q[2]) - np.log(q[3]))

    res["kldiv_fused"] = clock(lambda: V.vbmc_kldiv(vp, vp2, a.Nkl, seed=seed), a.reps, a.warmup, sync)
    res["kldiv_composed"] = clock(composed_kl, a.reps, a.warmup, sync)
    B1, _ = V.vp_rnd_rng_dump(seed, a.Nkl, D, vp["w"], True)
    B2, _ = V.vp_rnd_rng_dump(seed + 1, a.Nkl, D, vp2["w"], True)
    res["kldiv_host_given_the_blocks"] = clock(
        lambda: T.kldiv_terms(vp, vp2, T.rnd(vp, a.Nkl, True, True, B1, seed)[0], T.rnd(vp2, a.Nkl, True, True, B2, seed + 1)[0]), a.host_reps, 0, nosync)
    for k in ("moments", "kldiv"):
        res[k + "_fused_slowest_below_composed_fastest"] = bool(res[k + "_fused"]["max_ms"] < res[k + "_composed"]["min_ms"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

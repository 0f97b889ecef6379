"""CPU: the NumPy restatement of Step 1 of the IMIQR importance sampler and of the resampling (tests/_issetup_ref.py) against the oracle
(activesample_proposalpdf, vbmc_pdf_transformed, acq_islogf: 1e-12, the figure the oracle-vs-restatement tests here use) and against the
host Step 1 of vbmc_amd/acq.py fed the same points and uniforms; the margin of every resampling draw for the very case table
tests/test_gpu_issetup.py imports; and the host half of the library's generator (vbmc_acq_is_setup_rng_dump).

The EDGES table of tests/test_gpu_issetup_edges.py is held to the same conditions, and each edge case is shown here to reach the code
path it is named for: the run-out of the weights, the start without a finite weight, the full resampling wave, up to 32 components per
lane, the later trips of the box count, D = 32, and the seams of the prediction's row blocks on both Cholesky branches."""
import math

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _issetup_ref as T

TOL = 1e-12


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if np.size(a) else 0.0


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_every_draw_of_a_case_has_a_margin(name):
    c, ref = T.run_case(name)
    print("%s: smallest |u total - cdf| / total %.3e" % (name, ref["margin"]))
    assert ref["margin"] > T.DRAW_MARGIN
    assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False, True]
    assert not np.any(np.isnan(ref["lnw1"])) and not np.any(np.isnan(ref["x0"]))
    assert np.all(ref["x0"] >= ref["LB"]) and np.all(ref["x0"] <= ref["UB"])
    for s in range(c["S"]):
        assert np.unique(ref["idx0"][:, s]).size == c["W"]                 # without replacement: no case runs out of weights


def test_geometry_is_the_references():
    c, ref = T.run_case("D")
    X = c["gp"]["X"]
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    assert rel(ref["rect_delta"], 2 * np.std(X, axis=0, ddof=1)) < TOL
    assert rel(ref["LB"], np.min(X, axis=0) - 0.5 * diam) < TOL and rel(ref["UB"], np.max(X, axis=0) + 0.5 * diam) < TOL


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "P"])
def test_proposal_against_the_oracle(name):
    proposal_against_the_oracle(name)


def proposal_against_the_oracle(name):
    c, ref = T.run_case(name)
    gp, vp, Nvp, Nbox = c["gp"], c["vp"], c["Nvp"], c["Nbox"]
    w_vp = Nvp / (Nvp + Nbox)
    v4 = T.vp_is(vp) if Nvp > 0 else None
    with np.errstate(all="ignore"):
        lnw, fs2 = R.activesample_proposalpdf(ref["Xa1"], gp, v4, w_vp, ref["rect_delta"], "acqimiqr", vp, False)
    lnw = np.where(np.isfinite(lnw), lnw, -np.inf).T                        # :148
    fin = np.isfinite(lnw)
    assert np.array_equal(fin, np.isfinite(ref["lnw1"]))
    e = rel(ref["lnw1"][fin], lnw[fin])
    print("%s: lnw against activesample_proposalpdf %.2e, %d of %d finite" % (name, e, int(np.sum(fin)), fin.size))
    assert e < TOL and np.array_equal(fs2, ref["fs2a1"])
    if Nvp > 0:
        with np.errstate(divide="ignore"):
            lp = np.log(R.vbmc_pdf_transformed(v4, ref["Xa1"]))
        mine = T.mixture_lpdf(v4, ref["Xa1"])
        ok = np.isfinite(lp) & (lp > -600.0)                                 # (a denormal density has lost its digits)
        assert rel(mine[ok], lp[ok]) < TOL and np.all(mine[~np.isfinite(lp)] == -np.inf)
    _, lw = T.weights(ref["lpdf1"], ref["fmu1"], ref["fs2a1"])
    with np.errstate(invalid="ignore"):
        added = lw - ref["lnw1"].T
    assert rel(added[fin.T], R.acq_islogf("acqimiqr", "islogf2", None, ref["fmu1"], ref["fs2a1"])[fin.T]) < TOL
    if name == "P":
        assert np.all(ref["lnw1"][:, 0] == -np.inf) and ref["lpdf1"][0] == -np.inf and not np.any(ref["idx0"] == 0)
        assert np.all(np.isfinite(ref["lnw1"][:, 1:]))


# ---- the edge table
UNDERFLOW_EDGE = -745.13                                   # exp(x) rounds to zero below it, to the smallest denormal above


def draws_line(name, c, ref):
    d = ref["draws"]
    return "%s: margin %.3e  positive weights %s of %d  exact zeros %s  resets in front of draw %s" % (
        name, ref["margin"], [q["npos"] for q in d], c["Na1"], [q["zeros"] for q in d], [q["resets"] for q in d])


@pytest.mark.parametrize("name", sorted(T.EDGES))
def test_every_draw_of_an_edge_case_has_a_margin(name):
    c, ref = T.run_case(name)
    for k in ("Xa1", "lpdf1", "lnw1", "fs2a1", "fmu1"):
        assert not np.any(np.isnan(ref[k])), k
    if name in T.SEAM_NAMES:
        print("%s: Step 1 alone, N = %d: %d row blocks" % (name, c["N"], (c["N"] + 15) // 16))
        assert c["W"] == 0 and c["Nm"] == 0 and "idx0" not in ref and c["B"].size == (c["D"] + 1) * c["Na1"]
        return
    print(draws_line(name, c, ref))
    assert ref["margin"] > T.DRAW_MARGIN
    assert not np.any(np.isnan(ref["x0"]))
    assert np.all(ref["x0"] >= ref["LB"]) and np.all(ref["x0"] <= ref["UB"])
    assert np.all(ref["idx0"] >= 0) and np.all(ref["idx0"] < c["Na1"])
    for s, q in enumerate(ref["draws"]):
        # without replacement between two resets: the draws up to the first reset are distinct, and so are those of every stretch after
        cuts = [0] + [r for r in q["resets"] if r > 0] + [c["W"]]
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert np.unique(ref["idx0"][a:b, s]).size == b - a, (s, a, b)


def test_the_weights_run_out():
    """R: one positive weight under hyper-samples 0 and 2 -- the second of the W = 6 draws finds none and resets them to ones"""
    c, ref = T.run_case("R")
    W = c["W"]
    print(draws_line("R", c, ref))
    short = [s for s, q in enumerate(ref["draws"]) if 1 <= q["npos"] <= W - 1]
    assert short
    for s in short:
        q = ref["draws"][s]
        assert q["resets"] == [q["npos"]]                                    # the reset is taken, once, when the positive weights are used up
        lw = ref["lw"][:, s]
        assert np.all(lw[ref["idx0"][:q["npos"], s]] >= np.sort(lw)[-q["npos"]])          # the prefix: the points that had a weight
    dist = np.inf
    for s in range(c["S"]):
        lw = ref["lw"][:, s]
        rel_ = lw[np.isfinite(lw)] - np.max(lw)
        dist = min(dist, float(np.min(np.abs(rel_ - UNDERFLOW_EDGE))))
    print("R: the finite lw - max nearest to the underflow edge %.2f is %.1f away" % (UNDERFLOW_EDGE, dist))
    assert dist > 50.0


def test_the_weights_run_out_in_a_full_wave():
    """RL: Na1 = 256, the reset reaches the weights of every lane -- the draws behind it land beyond index 63, in lanes 16 and above"""
    c, ref = T.run_case("RL")
    print(draws_line("RL", c, ref))
    assert c["Na1"] == 256
    dist = np.inf
    for s, q in enumerate(ref["draws"]):
        assert 1 <= q["npos"] <= c["W"] - 1 and q["resets"] == [q["npos"]]
        after = ref["idx0"][q["npos"]:, s]
        print("RL: hyper-sample %d draws from the reset weights %s" % (s, after.tolist()))
        assert np.sum(after >= 64) >= 2 and np.any(after % 4 != 0)
        lw = ref["lw"][:, s]
        dist = min(dist, float(np.min(np.abs((lw[np.isfinite(lw)] - np.max(lw)) - UNDERFLOW_EDGE))))
    print("RL: the finite lw - max nearest to the underflow edge is %.1f away" % dist)
    assert dist > 50.0


def test_weights_underflow_without_running_out():
    c, ref = T.run_case("R9")
    print(draws_line("R9", c, ref))
    for q in ref["draws"]:
        assert q["npos"] >= c["W"] and q["zeros"] >= 1 and q["resets"] == []


def test_no_finite_weight_at_all():
    c, ref = T.run_case("O")
    print(draws_line("O", c, ref))
    dead = [s for s in range(c["S"]) if not np.any(np.isfinite(ref["lw"][:, s]))]
    assert dead == [2]                                                         # (a Cholesky hyper-sample: its fs2 stays well conditioned)
    assert ref["draws"][2]["resets"] == [0] and ref["draws"][2]["npos"] == 0                  # ones from the first draw
    assert np.all(ref["fmu1"][:, 2] == -np.inf) and np.all(np.isfinite(ref["lpdf1"]))
    assert all(q["resets"] == [] and q["npos"] == c["Na1"] for s, q in enumerate(ref["draws"]) if s != 2)


def test_the_full_resampling_wave():
    c, ref = T.run_case("L")
    assert c["Na1"] == 256 and (c["Na1"] + 15) // 16 == 16
    top = int(np.max(ref["idx0"]))
    print("L: largest drawn index %d (lane %d), indices with idx %% 4 == 3: %d, 4K = %d, N = %d" % (
        top, top // 4, int(np.sum(ref["idx0"] % 4 == 3)), 4 * c["K"], c["N"]))
    assert top >= 192 and np.any(ref["idx0"] % 4 == 3)
    assert all(q["npos"] == 256 for q in ref["draws"])                         # every lane's four weights are positive
    assert 4 * c["K"] == 64 and c["N"] > 128                                   # one component per lane; a third trip of the box count


def test_widths_of_the_edge_cases():
    """4K against the wave (64 lanes), N against the box count's stride, D and W at their limits"""
    L, W, K = (T.run_case(n)[0] for n in ("L", "W", "K"))
    assert (W["D"], W["W"], W["Na1"], 4 * W["K"], W["N"]) == (32, 66, 129, 68, 70)     # D = 32: lane < D and tid < D at the limit
    assert 4 * K["K"] == 2048 == 32 * 64                                       # 32 components per lane
    assert L["K"] == 16 and W["K"] == 17                                       # the exact wave width and one more
    assert L["N"] == 130 and W["N"] == 70                                      # a third / a second trip of n = lane, lane + 64, ...
    assert [bool(p["Lchol"]) for p in W["gp"]["post"]] == [True]               # the knob "no low-noise hyper-sample"


@pytest.mark.parametrize("name", ["L", "W", "K"])
def test_components_fall_in_all_four_replicas(name):
    c, ref = T.run_case(name)
    comp = T.components(c["B"], c["vp"], c["Nvp"])
    per = np.bincount(comp // c["K"], minlength=4)
    print("%s: points per replica of the smoothed mixture %s, components used %d of %d" % (name, per.tolist(), np.unique(comp).size, 4 * c["K"]))
    assert np.all(per > 0) and np.max(comp) < 4 * c["K"]


def test_a_box_point_draws_the_first_and_the_last_input():
    c, ref = T.run_case("L")
    j = T.box_inputs(c["B"], c["D"], c["N"], c["Nvp"], c["Nbox"])
    print("L: box points around input 0: %d, around input N - 1: %d" % (int(np.sum(j == 0)), int(np.sum(j == c["N"] - 1))))
    assert j[0] == c["N"] - 1 and j[1] == 0                                    # planted: the largest and the smallest uniform there is
    rd = ref["rect_delta"]
    X = c["gp"]["X"]
    assert np.all(np.abs(ref["Xa1"][c["Nvp"]] - X[-1]) <= rd) and np.all(np.abs(ref["Xa1"][c["Nvp"] + 1] - X[0]) <= rd)


def branch_counts(ref):
    f0, f1 = np.isfinite(ref["t0"]), np.isfinite(ref["t1"])
    return {"both": int(np.sum(f0 & f1)), "mixture only": int(np.sum(f0 & ~f1)), "box only": int(np.sum(~f0 & f1)), "neither": int(np.sum(~f0 & ~f1))}


def test_each_combination_of_the_two_proposal_terms_occurs():
    """(t0, t1) of k_is_proposal: both finite in A; the mixture alone in W (Nbox > 0: points of the mixture outside every box) and in
    C (Nbox = 0); the boxes alone in B (Nvp = 0); neither in P (the planted point)"""
    seen = {}
    for name in sorted(T.CASES) + sorted(T.EDGES):
        _, ref = T.run_case(name)
        seen[name] = branch_counts(ref)
        print("%s: %s" % (name, seen[name]))
    assert seen["A"]["both"] > 0
    assert seen["W"]["mixture only"] > 0 and seen["W"]["both"] > 0 and seen["C"]["mixture only"] > 0
    assert seen["B"]["box only"] > 0
    assert seen["P"]["neither"] == 1


@pytest.mark.parametrize("name", sorted(T.EDGES))
def test_edge_proposal_against_the_oracle(name):
    proposal_against_the_oracle(name)


@pytest.mark.parametrize("name", T.SEAM_NAMES)
def test_seam_cases_have_both_cholesky_branches(name):
    c, ref = T.run_case(name)
    assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False]
    assert c["Na1"] == 48 and np.all(np.isfinite(ref["lnw1"])) and np.all(np.isfinite(ref["lpdf1"]))
    nblk = (c["N"] + 15) // 16
    print("%s: %d row blocks, %d snake periods begun, N %% 16 = %d" % (name, nblk, (nblk + 15) // 16, c["N"] % 16))


def test_the_seams_are_the_kernels():
    """one block; a full block; eight blocks and the ninth (the first snake turn); sixteen and the seventeenth (the second period); the
    top of the resident range.  inv(L') is kept while the triangular solves run 16 columns wide: (17 Np + 64 * 17) doubles within the
    160 KB of LDS (trsm_cw_for), Np <= 1136 -- the prediction's own tile (16 Np doubles, 156 KB at the most) would reach N = 1248 -- and
    k_is_pred's 16 Np doubles of dynamic LDS beside 3 072 B of static LDS fit there with room to spare"""
    blocks = [(n + 15) // 16 for n in T.N_SEAMS]
    assert blocks == [1, 1, 8, 9, 16, 17, 71]
    assert [n % 16 == 0 for n in T.N_SEAMS] == [False, True, True, False, True, False, True]
    top, nxt = T.N_SEAMS[-1], 16 * ((T.N_REFUSED + 15) // 16)
    assert T.N_REFUSED == top + 1 and top % 16 == 0
    assert (17 * top + 64 * 17) * 8 <= 160 * 1024 < (17 * nxt + 64 * 17) * 8
    assert 16 * top * 8 + 3072 <= 160 * 1024 and 16 * top * 8 <= 156 * 1024


class BlockRng:
    """numpy's Generator calls of the host Step 1, answered from the block in the block's own order"""

    def __init__(self, c):
        self.c, self.B, self.drawn = c, c["B"], 0
        self.D1 = c["D"] + 1

    def choice(self, K, size, p):
        cdf = np.cumsum(p)
        return np.array([min(int(np.sum(cdf < self.B[self.D1 * i] * cdf[-1])), K - 1) for i in range(size)])

    def standard_normal(self, shape):
        return np.stack([self.B[self.D1 * i + 1:self.D1 * (i + 1)] for i in range(shape[0])])

    def integers(self, lo, hi, size):
        return np.array([min(int(math.floor(self.B[self.D1 * (self.c["Nvp"] + i)] * hi)), hi - 1) for i in range(size)])

    def random(self, shape=None):
        if shape is not None:
            return np.stack([self.B[self.D1 * (self.c["Nvp"] + i) + 1:self.D1 * (self.c["Nvp"] + i + 1)] for i in range(shape[0])])
        self.drawn += 1
        return self.B[self.D1 * self.c["Na1"] + self.drawn - 1]


class Captured(Exception):
    pass


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_step_one_picks_the_same_walkers(name, monkeypatch):
    from vbmc_amd import acq

    c, ref = T.run_case(name)
    gp, S = c["gp"], c["S"]

    def pred(gp_, Xs, engine):
        o = R.gplite_pred(gp_, np.asarray(Xs), None, None, True)
        return tuple(np.asarray(v).reshape(np.asarray(Xs).shape[0], S) for v in o)

    def capture(logp, x0, *a, **k):
        raise Captured(x0.copy())

    monkeypatch.setattr(acq, "gplite_pred_device", pred)
    monkeypatch.setattr(acq, "ensemble_slice_sample", capture)
    opts = {"ActiveImportanceSamplingMCMCSamples": c["Nm"], "ActiveImportanceSamplingVPSamples": c["Nvp"], "ActiveImportanceSamplingBoxSamples": c["Nbox"]}
    rng = BlockRng(c)
    with pytest.raises(Captured) as e:
        acq.activeimportancesampling_vbmc(c["vp"], gp, "acqimiqr_vbmc", None, opts, rng=rng, engine=object())
    x0 = e.value.args[0]
    assert rng.drawn == c["W"] * S
    err = rel(x0, ref["x0"])
    print("%s: the host's starting walkers against the restatement's %.2e" % (name, err))
    assert x0.shape == ref["x0"].shape and err < TOL


def dump(seed, D, S, W, Nvp, Nbox):
    import __graft_entry__ as g

    g.build()
    from vbmc_amd.acq import importance_setup_rng_dump

    return importance_setup_rng_dump(seed, D, S, W, Nvp, Nbox)


def test_rng_dump_layout_and_determinism():
    D, S, W, Nvp, Nbox = 3, 2, 8, 5, 4
    a, b = dump(7, D, S, W, Nvp, Nbox), dump(7, D, S, W, Nvp, Nbox)
    assert a.size == T.block_len(D, S, W, Nvp, Nbox) and np.array_equal(a, b) and not np.array_equal(dump(8, D, S, W, Nvp, Nbox), a)
    pts = a[:(D + 1) * (Nvp + Nbox)].reshape(Nvp + Nbox, D + 1)
    uni = np.concatenate([pts[:, 0], pts[Nvp:, 1:].reshape(-1), a[(D + 1) * (Nvp + Nbox):]])
    assert np.all(uni > 0.0) and np.all(uni < 1.0) and np.unique(uni).size == uni.size
    z = pts[:Nvp, 1:]
    assert np.all(np.isfinite(z)) and np.any(z < 0.0) and np.any(z > 0.0)
    # a point's values do not depend on how many points follow it; the draws are keyed by (ensemble, draw)
    more = dump(7, D, S + 1, W, Nvp, Nbox)
    assert np.array_equal(more[:(D + 1) * (Nvp + Nbox)], a[:(D + 1) * (Nvp + Nbox)])
    assert np.array_equal(more[(D + 1) * (Nvp + Nbox):(D + 1) * (Nvp + Nbox) + W * S], a[(D + 1) * (Nvp + Nbox):])
    big = dump(3, 10, 1, 0, 200, 0)[: 11 * 200].reshape(200, 11)[:, 1:]
    assert abs(float(np.mean(big))) < 0.1 and abs(float(np.std(big)) - 1.0) < 0.1
    from vbmc_amd import _lib

    assert _lib.load().vbmc_acq_is_setup_rng_dump(1, 0, 1, 4, 1, 1, None) == 1

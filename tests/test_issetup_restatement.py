"""CPU: the NumPy restatement of Step 1 of the IMIQR importance sampler and of the resampling (tests/_issetup_ref.py) against the oracle
(activesample_proposalpdf, vbmc_pdf_transformed, acq_islogf: 1e-12, the figure the oracle-vs-restatement tests here use) and against the
host Step 1 of vbmc_amd/acq.py fed the same points and uniforms; the margin of every resampling draw for the very case table
tests/test_gpu_issetup.py imports; and the host half of the library's generator (vbmc_acq_is_setup_rng_dump)."""
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

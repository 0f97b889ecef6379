"""CPU: the NumPy restatement of the indexed-uniform ensemble slice sampler (tests/_issample_ref.py) and the host half of the library's
generator (vbmc_acq_is_sample_rng_dump).  The margin condition is asserted for the very case table tests/test_gpu_issample.py imports: no
GPU case can hide a flipped decision behind a near-tie."""
import math

import numpy as np
import pytest

from tests import _issample_ref as I


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_every_decision_of_a_case_has_a_margin(name):
    c, ref = I.run_case(name)
    print("%s: margin %.3e funccount %d half-moves %d outside %d" % (name, ref["margin"], ref["funccount"], ref["halfmoves"], ref["outside"]))
    assert ref["margin"] > I.MARGIN
    assert ref["halfmoves"] == c["M"] <= c["U"].shape[3]
    assert np.all(ref["Xa"] >= c["LB"][None, :, None]) and np.all(ref["Xa"] <= c["UB"][None, :, None])
    if name == "C":
        assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False]
    if name == "E":
        assert ref["outside"] > 0


@pytest.mark.parametrize("name", sorted(I.EDGE_CASES))
def test_every_decision_of_an_edge_case_has_a_margin(name):
    """the chain cases of tests/test_gpu_issetup_edges.py: N = 16, 129, 257 and 1136, the seams of the prediction's row blocks"""
    c, ref = I.run_case(name)
    lchol = [bool(p["Lchol"]) for p in c["gp"]["post"]]
    print("%s: N %d (%d row blocks) margin %.3e funccount %d half-moves %d outside %d Lchol %s" % (
        name, c["N"], (c["N"] + 15) // 16, ref["margin"], ref["funccount"], ref["halfmoves"], ref["outside"], lchol))
    assert ref["margin"] > I.MARGIN
    assert ref["halfmoves"] == c["M"] <= c["U"].shape[3]
    assert np.all(ref["Xa"] >= c["LB"][None, :, None]) and np.all(ref["Xa"] <= c["UB"][None, :, None])
    assert c["N"] == {"G": 16, "H": 129, "J": 257, "T": 1136}[name]
    assert lchol == ([True] if name == "G" else [True, False])


def gauss_target(mu, prec):
    def logp(P, e):
        d = P - mu
        return -0.5 * np.einsum("ni,ij,nj->n", d, prec, d)

    return logp


def test_spec_changes_nothing_but_the_evaluations_made():
    rng = np.random.default_rng(4)
    S, W, D, Nm = 2, 8, 3, 20
    logp = gauss_target(np.zeros(D), np.eye(D))
    x0 = rng.standard_normal((S, W, D))
    LB, UB = np.full(D, -2.5), np.full(D, 2.5)            # tight enough for proposals to leave the box
    x0 = np.clip(x0, LB, UB)
    U = rng.random((I.SLOTS, W // 2, S, I.halfmoves_needed(Nm, W // 2)))
    runs = [I.sample(logp, x0, LB, UB, Nm, U, spec=s) for s in (1, 2, 3, 4)]
    assert runs[0]["performed"] == runs[0]["funccount"] and runs[0]["outside"] > 0
    for r in runs[1:]:
        assert np.array_equal(r["Xa"], runs[0]["Xa"]) and np.array_equal(r["logp"], runs[0]["logp"])
        assert r["funccount"] == runs[0]["funccount"] and r["performed"] > runs[0]["performed"]


def test_gaussian_target_moments():
    """4 000 recorded samples of a correlated 2-D Gaussian: mean and covariance within 0.15 (tests/test_importance_sampler.py's kind of check)"""
    rng = np.random.default_rng(0)
    mu = np.array([0.5, -1.0])
    cov = np.array([[1.0, 0.6], [0.6, 1.5]])
    logp = gauss_target(mu, np.linalg.inv(cov))
    S, W, Nm = 4, 6, 1000
    x0 = mu + rng.standard_normal((S, W, 2))
    U = rng.random((I.SLOTS, W // 2, S, I.halfmoves_needed(Nm, W // 2)))
    r = I.sample(logp, x0, np.full(2, -50.0), np.full(2, 50.0), Nm, U, spec=4)
    X = np.concatenate([r["Xa"][:, :, s] for s in range(S)], axis=0)
    assert X.shape == (4000, 2)
    em, ec = np.max(np.abs(np.mean(X, axis=0) - mu)), np.max(np.abs(np.cov(X, rowvar=False) - cov))
    print("mean error %.3f covariance error %.3f" % (em, ec))
    assert em < 0.15 and ec < 0.15
    assert np.allclose(r["logp"][0], logp(r["Xa"][:, :, 0], 0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("thin,burnin", [(1, None), (3, None), (2, 0), (2, 7)])
def test_records_follow_the_host_samplers_rule(thin, burnin):
    """the recorded walkers are the moves burnin + thin, burnin + 2 thin, ... counted one per walker of each finished half-move"""
    rng = np.random.default_rng(2)
    S, W, D, Nm = 1, 6, 2, 9
    H = W // 2
    logp = gauss_target(np.zeros(D), np.eye(D))
    x0 = rng.standard_normal((S, W, D))
    M = I.halfmoves_needed(Nm, H, thin, burnin)
    U = rng.random((I.SLOTS, H, S, M))
    r = I.sample(logp, x0, np.full(D, -9.0), np.full(D, 9.0), Nm, U, thin=thin, burnin=burnin)
    assert r["halfmoves"] == M
    b = int(math.ceil(thin * Nm / 2)) if burnin is None else burnin
    # replay the walkers half-move by half-move from shorter runs: the k-th record is walker (move - 1) % H of half-move (move - 1) // H
    for k in range(Nm):
        move = b + (k + 1) * thin
        m, j = (move - 1) // H, (move - 1) % H
        # a run that records every move (thin 1, no burn-in) holds the walker of that move at index move - 1
        full = I.sample(logp, x0, np.full(D, -9.0), np.full(D, 9.0), move, U[:, :, :, : m + 1], thin=1, burnin=0)
        assert np.array_equal(full["Xa"][move - 1, :, 0], r["Xa"][k, :, 0]), (k, m, j)
    with pytest.raises(ValueError, match="uniform block exhausted"):
        I.sample(logp, x0, np.full(D, -9.0), np.full(D, 9.0), Nm, U[:, :, :, : M - 1], thin=thin, burnin=burnin)


def dump(seed, S, H, M):
    import __graft_entry__ as g

    g.build()
    from vbmc_amd.acq import importance_sample_rng_dump

    return importance_sample_rng_dump(seed, S, H, M)


def test_rng_dump_is_deterministic_inside_the_unit_interval_and_prefix_stable():
    a, b = dump(7, 3, 4, 5), dump(7, 3, 4, 5)
    assert a.shape == (64, 4, 3, 5) and np.array_equal(a, b)
    assert np.all(a > 0.0) and np.all(a < 1.0)
    assert np.array_equal(dump(7, 3, 4, 6)[:, :, :, :5], a)
    assert not np.array_equal(dump(8, 3, 4, 5), a)
    big = dump(1, 2, 3, 27)                                # 64 * 3 * 2 * 27 = 10 368 values
    assert big.size >= 10000 and np.unique(big.reshape(-1)[:10000]).size == 10000
    assert abs(float(np.mean(big)) - 0.5) < 0.02

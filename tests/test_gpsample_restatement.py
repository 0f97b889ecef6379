"""CPU: the restatement of the surrogate sampler (tests/_gpsample_ref.py) reaches, on every case of its table, the path the case is
there for, with every consumed comparison further than MARGIN from its slice level -- so that a device run that differs in the last
bits takes the same decisions -- and, in the noise cases, with every draw's two smallest distances further apart than GAP, so that the
first-minimum rule cannot flip.  The seeds of the table were chosen here, on the restatement alone."""
import numpy as np
import pytest

from tests import _gpsample_ref as G


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_case_reaches_its_path(name):
    c, r = G.run_case(name)
    print("%s: margin %.2e  funccount %d  halfmoves %d  outside %d  active %d  inactive %d" % (name, r["margin"], r["funccount"], r["halfmoves"],
                                                                                            r["outside"], r["active"], r["inactive"]))
    assert r["margin"] > G.MARGIN
    assert r["halfmoves"] <= c["M"]
    assert r["Xa"].shape == (c["Nm"], c["D"], c["E"]) and r["X"].shape == (c["Ns"], c["D"])
    assert np.all(np.isfinite(r["logp"]))
    post = c["gp"]["post"]
    if name == "A":
        assert len(post) == 1 and not np.isfinite(c["VarThresh"]) and c["beta"] == 0
    if name == "B":
        assert len(post) == 3 and r["active"] > 0 and r["inactive"] > 0
        # the two ensembles do not advance in step: their evaluation counts differ
        one = [G.I.sample(G.log_gpfun(c["gp"], c["VarThresh"], c["beta"]), c["x0"][e:e + 1], c["LB"], c["UB"], c["Nm"], c["U"][:, :, e:e + 1],
                          thin=c["thin"], burnin=c["burnin"])["funccount"] for e in range(2)]
        assert one[0] != one[1] and sum(one) == r["funccount"]
    if name == "C":
        assert [bool(p["Lchol"]) for p in post] == [True, False] and c["beta"] == 0.5
    if name == "D":
        assert 2 * 3 * c["H"] == 198 and (c["D"] + 3) // 4 == 8
    if name == "E":
        assert r["outside"] > 0 and c["Nm"] == 5 and c["Nm"] * c["E"] - c["Ns"] == 2
        assert np.array_equal(r["X"][5], r["Xa"][1, :, 0]) and np.array_equal(r["X"][22], r["Xa"][4, :, 2])
    if name == "F":
        assert c["Nm"] == 300 > 256
    if name == "G":
        assert c["N"] == 1136 and sorted(bool(p["Lchol"]) for p in post) == [False, True]


def test_interleave():
    Xt = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4)
    X = G.interleave(Xt, 10)
    assert X.shape == (10, 2)
    for r in range(10):
        assert np.array_equal(X[r], Xt[r // 4, :, r % 4])


@pytest.mark.parametrize("name", sorted(G.VP_CASES))
@pytest.mark.parametrize("Nnn", [G.NNN, 20000])
def test_noise_cases_have_no_near_ties(name, Nnn):
    from tests import _vptools_ref as T
    from vbmc_amd import vptools
    from vbmc_amd.gplite import gp_surrogate_sample_rng_dump  # noqa: F401  (the mirror of the feature)

    c = G.build_vp_case(name)
    vp, nz = c["vp"], c["noise"]
    B, _ = vptools.vp_rnd_rng_dump(G.VP_SEED + 1, Nnn, vp["D"], vp["w"], False)
    _, _, Y = T.rnd(vp, Nnn, False, False, B, G.VP_SEED + 1)
    pos, avg, vt, gap = G.noise_estimate(Y, nz["gplengthscale"], nz["X_rescaled"], nz["sn2new"])
    print("%s Nnn %d: gap %.2e  sn2_avg %.6f  distinct rows %d" % (name, Nnn, gap, avg, len(set(pos.tolist()))))
    assert gap > G.GAP
    assert len(set(pos.tolist())) > 1 and vt == max(1.0, avg)
    assert (avg > 1.0) == (name == "C")                # both sides of max(1, sn2_avg): B stays at 1, C takes the estimate

"""CPU: the preconditions of the GPU trajectory comparison (tests/test_gpu_acqsearch_iqr.py) hold for every case of
tests/_acqsearch_iqr_ref.py on the restatement's own 12-generation trajectory over the oracle's IQR acquisition functions: neighbouring
sorted values further apart than 1e-6 (1 + |F|) -- the comparison's tolerance is 1e-8 on that scale --, every visited value finite and,
with the variance regulariser on, the smallest vtot visited above TolGPVar (below it the regulariser amplifies a prediction's rounding by
TolGPVar / vtot^2; tests/test_gpu_acq.py leaves such points out for the same reason)."""
import numpy as np
import pytest

from tests import _acqsearch_iqr_ref as I


@pytest.mark.parametrize("name", sorted(I.iqr_cases()))
def test_reference_trajectory_meets_the_preconditions(name):
    D, N, S, Na, fun, reg, face, popsize, _ = I.iqr_cases()[name]
    c = I.build_case(name)
    if S == 3:
        assert [bool(p["Lchol"]) for p in c["gp"]["post"]] == [True, False, True]
    ref = I.run_case(c)
    gap, vmin, finite, ok = I.preconditions(c, ref)
    print("%s: rank gap %.2e, smallest vtot %.2e" % (name, gap, vmin))
    assert ref["generations"] == I.GENS and ref["popsize"] == c["lam"] == (popsize or I.A.default_popsize(D))
    assert gap > 1e-6 and finite
    assert all(np.all(np.isfinite(t["F"])) for t in ref["trace"])
    if reg:
        assert vmin > c["st"]["TolGPVar"]
    assert ok
    if face:
        assert sum(int(np.sum((t["X"] == c["LB"][:, None]) | (t["X"] == c["UB"][:, None]))) for t in ref["trace"]) > 0
    if fun == "acqimiqr":
        ais = c["st"]["ActiveImportanceSampling"]
        assert ais["Xa"].ndim == 3 and np.any(ais["lnw"] != 0)

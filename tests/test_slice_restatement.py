"""CPU: pins the NumPy restatement of slicesamplebnd (tests/_slice_ref.py) that the device chain is compared with, and the new
entry point's presence in the header, the built library and the ctypes binding."""
import ctypes
import os
import re

import numpy as np

from tests._slice_ref import make_block, slicesamplebnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_form_target_moments():
    """Independent Gaussians inside wide bounds: 4000 recorded samples after burn-in, mean and standard deviation within 4 standard
    errors of the truth (the standard errors use the chain's own integrated autocorrelation time; seed fixed)."""
    mu = np.array([0.5, -2.0, 3.0])
    sd = np.array([1.0, 0.3, 2.5])
    logf = lambda x: float(-0.5 * np.sum(((x - mu) / sd) ** 2))  # noqa: E731
    N, burn, D = 4000, 300, 3
    perms, U = make_block(np.random.default_rng(20240611), N + burn, D, 60)
    s, f, out = slicesamplebnd(logf, mu + 0.1, N, np.ones(D), -50.0 * np.ones(D), 50.0 * np.ones(D), {"Burnin": burn, "Thin": 1}, perms, U)
    assert s.shape == (N, D) and np.all(np.isfinite(f))
    assert np.allclose(f, [logf(x) for x in s])
    for d in range(D):
        x = s[:, d]
        c = x - x.mean()
        acf = np.array([np.dot(c[: N - k], c[k:]) / np.dot(c, c) for k in range(1, 40)])
        pos = np.argmax(acf < 0.05) if np.any(acf < 0.05) else acf.size
        tau = 1.0 + 2.0 * float(np.sum(acf[:pos]))
        neff = N / tau
        assert tau < 3.0 and neff > 500, (d, tau)      # the inflation stays small: it cannot hide a sampler that does not mix
        se_mean = sd[d] / np.sqrt(neff)
        se_sd = sd[d] / np.sqrt(2.0 * neff)
        assert abs(x.mean() - mu[d]) < 4 * se_mean, (d, x.mean(), mu[d], se_mean)
        assert abs(x.std(ddof=1) - sd[d]) < 4 * se_sd, (d, x.std(ddof=1), sd[d], se_sd)
    assert out["funccount"] > (N + burn) * D          # at least one evaluation per coordinate update, plus the one at x0


def test_fixed_coordinate_bounds_and_nonadaptive_widths():
    mu = np.array([0.0, 1.0, -1.0, 0.3])
    logf = lambda x: float(-0.5 * np.sum((x - mu) ** 2))  # noqa: E731
    LB = np.array([-0.4, 1.0, -np.inf, 0.25])
    UB = np.array([0.6, 1.0, 0.0, np.inf])
    x0 = np.array([0.1, 1.0, -0.5, 0.26])
    N, burn, D = 300, 40, 4
    perms, U = make_block(np.random.default_rng(7), N + burn, D, 80)
    w0 = np.array([0.7, 0.2, 3.0, 1.5])
    s, f, out = slicesamplebnd(logf, x0, N, w0, LB, UB, {"Burnin": burn, "Thin": 1, "Adaptive": False}, perms, U)
    assert np.all(s[:, 1] == 1.0)                                       # a fixed coordinate is never moved
    assert np.all(s >= LB) and np.all(s <= UB)                          # samples never leave [LB, UB]
    assert s[:, 0].min() < -0.3 and s[:, 0].max() > 0.5                 # ... and reach towards both ends of a tight box
    exp_w = w0.copy()
    exp_w[1] = 1.0                                                      # (irrelevant width of the fixed coordinate, :185)
    assert np.array_equal(out["widths"], exp_w)                         # Adaptive = false: the widths come back unchanged
    # adaptive: widths move, thinning keeps every Thin-th sweep of the same chain
    s1, _, o1 = slicesamplebnd(logf, x0, N, w0, LB, UB, {"Burnin": burn, "Thin": 1}, perms, U)
    free = LB != UB                     # (a fixed coordinate's zero variance makes its -- irrelevant -- width 0 at the end of burn-in, :347)
    assert not np.array_equal(o1["widths"], exp_w) and np.all(o1["widths"][free] > 0) and np.all(np.isfinite(o1["widths"]))
    n3 = (N - 1) // 3 + 1
    s3, _, _ = slicesamplebnd(logf, x0, n3, w0, LB, UB, {"Burnin": burn, "Thin": 3}, perms, U)
    assert np.array_equal(s3, s1[::3][:n3])


def test_nan_target_is_a_rejection_and_counts():
    calls = {"n": 0}

    def logf(x):
        calls["n"] += 1
        return np.nan if x[0] > 1.0 else float(-0.5 * x[0] ** 2)

    perms, U = make_block(np.random.default_rng(3), 200, 1, 80)
    s, _, out = slicesamplebnd(logf, np.array([0.0]), 200, np.array([4.0]), None, None, {"Burnin": 0, "Adaptive": False}, perms, U)
    assert np.all(s <= 1.0) and out["funccount"] == calls["n"]


def test_header_library_and_binding_have_the_entry_point():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"vbmc_status\s+vbmc_gp_slice_sample\s*\(", code) and re.search(r"vbmc_status\s+vbmc_slice_rng_dump\s*\(", code)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vbmc_gp_slice_sample") and hasattr(lib, "vbmc_slice_rng_dump")
    bound = _lib.load()
    assert bound.vbmc_gp_slice_sample.argtypes is not None and bound.vbmc_slice_rng_dump.argtypes is not None
    assert ctypes.sizeof(_lib.SliceArgs) % 8 == 0
    import vbmc_amd

    assert callable(vbmc_amd.slicesamplebnd_gp) and callable(vbmc_amd.gplite_train_sample)
    # the dump hook is a pure host function: the indexed block of a seed, reproducible, uniforms inside (0, 1), rows are permutations
    p1, u1 = vbmc_amd.slice_rng_dump(11, 5, 7, 4)
    p2, u2 = vbmc_amd.slice_rng_dump(11, 5, 7, 4)
    p3, u3 = vbmc_amd.slice_rng_dump(12, 5, 7, 4)
    assert np.array_equal(p1, p2) and np.array_equal(u1, u2) and not np.array_equal(u1, u3)
    assert u1.shape == (5, 7, 6) and np.all((u1 > 0) & (u1 < 1))
    assert all(sorted(r) == list(range(7)) for r in p1) and len({tuple(r) for r in p1}) > 1
    # a longer block extends a shorter one: slot (sweep, idd, k) does not depend on Kmax
    _, u9 = vbmc_amd.slice_rng_dump(11, 5, 7, 9)
    assert np.array_equal(u9[:, :, :6], u1)

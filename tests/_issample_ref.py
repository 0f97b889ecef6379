"""The indexed-uniform ensemble slice sampler of vbmc_acq_is_sample (include/vbmc_hip.h), restated in NumPy one candidate at a time with
the target passed as a callable, and the shared case table of tests/test_issample_restatement.py (CPU) and tests/test_gpu_issample.py.

All randomness is  U[slot, j, e, m]  (64 x H x S x M; m the half-move counted from 0, half m mod 2 moves, e the ensemble, j the position
inside the moving half):  slot 0 a = floor(u H), 1 b = (a + 1 + floor(u (H - 1))) mod H, 2 level y = logp(x) + log u, 3 L = -u, R = L + 1,
4 + q the q-th shrink proposal t = L + u (R - L), a rejected t < 0 becomes L, otherwise R.  The left end after k steps is L - k, the right
end R + k, a candidate is x + t (x_other[b] - x_other[a]); every operation is one rounded NumPy operation.

``spec`` candidates of a walker are handed to the target in one call (2 spec while stepping out): an end stops at the first step below the
level, the shrinkage accepts the first proposal above it, what lies behind was evaluated for nothing.  ``funccount`` counts the in-bounds
evaluations spec = 1 consumes, ``performed`` all in-bounds evaluations made; ``margin`` is the smallest |value - level| / max(1, |level|)
over the comparisons that were consumed.

Cases (D, N, S, W, Nm, thin, meanfun, noisy, low_noise, tight, seed): the smallest shapes at which each piece can go wrong
  A  meanfun 0, N = 33 no multiple of 16, H = 3: the first H where slot 1 has a choice
  B  meanfun 4, noisefun (1, 1, 0) with s2, thin 2
  C  meanfun 1, two hyper-samples: one with sn2 < 1e-6 (Lchol = false) beside a Cholesky one
  D  D = 32, H = 33: 198 candidates at spec 3 -- twelve full 16-point tiles and a partial one; QS = 8
  E  H = 2, the degenerate direction pick; bounds so tight that some proposals fall outside them
  F  N = 530: the cross-kernel tile needs more than 64 KB of LDS (the prediction kernel's opted-in dynamic allocation), N no multiple of 16

Edge cases (EDGE_CASES, tests/test_gpu_issetup_edges.py): the seams of k_is_pred's row blocks, walked by the chain
  G  N = 16: one row block, seven of the eight waves idle, N an exact multiple of 16
  H  N = 129: nine row blocks, the first turn of the snake order; a Cholesky and a low-noise hyper-sample
  J  N = 257: seventeen row blocks, the snake's second period
  T  N = 1136: the top of the range in which inv(L') stays resident, 71 row blocks on both branches
"""
import math

import numpy as np

from oracle import vbmc_ref as R

U_IQR = 0.6745
SLOTS = 64
MARGIN = 1e-6


def sample(logp, x0, LB, UB, Nm, U, *, thin=1, burnin=None, spec=1, max_steps=20, max_shrink=60):
    """x0: S x W x D.  logp(P (n x D), e) -> n values of ensemble e's target.  Returns a dict: Xa (Nm x D x S), logp (S x Nm), funccount,
    performed, margin, halfmoves, outside (candidates that fell outside the box)."""
    x = np.array(x0, dtype=np.float64, copy=True)
    S, W, D = x.shape
    H = W // 2
    assert W >= 4 and W % 2 == 0
    LB = np.asarray(LB, dtype=np.float64).reshape(D)
    UB = np.asarray(UB, dtype=np.float64).reshape(D)
    burnin = int(math.ceil(thin * Nm / 2)) if burnin is None else int(burnin)
    out = {"Xa": np.zeros((Nm, D, S)), "logp": np.zeros((S, Nm)), "funccount": 0, "performed": 0, "margin": np.inf, "halfmoves": 0, "outside": 0}

    def values(P, e):
        """the target at the rows of P inside the box (-inf outside, no evaluation); a value that is not finite is -inf"""
        P = np.asarray(P).reshape(-1, D)
        inb = np.all((P >= LB) & (P <= UB), axis=1)
        v = np.full(P.shape[0], -np.inf)
        out["outside"] += int(np.sum(~inb))
        if np.any(inb):
            r = np.asarray(logp(P[inb], e), dtype=np.float64).reshape(-1)
            v[inb] = np.where(np.isfinite(r), r, -np.inf)
        return v, inb

    def above(v, y):
        if np.isfinite(v):
            out["margin"] = min(out["margin"], abs(v - y) / max(1.0, abs(y)))
        return v > y

    for e in range(S):
        lp, inb = values(x[e], e)
        assert np.all(inb), "a starting point is outside the box"
        if not np.all(np.isfinite(lp)):
            raise ValueError("a starting point has zero density")
        out["funccount"] += W
        out["performed"] += W
        moved = nrec = m = 0
        while nrec < Nm:
            if m >= U.shape[3]:
                raise ValueError("uniform block exhausted")
            mine = np.arange(H) + (m % 2) * H
            other = np.arange(H) + (1 - m % 2) * H
            xo = x[e, other].copy()
            for j in range(H):
                u = U[:, j, e, m]
                a = min(int(math.floor(u[0] * H)), H - 1)
                b = (a + 1 + min(int(math.floor(u[1] * (H - 1))), H - 2)) % H
                v = xo[b] - xo[a]
                xc = x[e, mine[j]].copy()
                y = lp[mine[j]] + math.log(u[2])
                L0 = -u[3]
                R0 = L0 + 1.0
                kL = kR = steps = 0
                gL = gR = True
                while steps < max_steps and (gL or gR):
                    ns = min(spec, max_steps - steps)
                    ts = ([L0 - float(kL + q) for q in range(ns)] if gL else []) + ([R0 + float(kR + q) for q in range(ns)] if gR else [])
                    val, inb = values(np.stack([xc + t * v for t in ts]), e)
                    out["performed"] += int(np.sum(inb))
                    c = 0
                    for side in ("L", "R"):
                        if not (gL if side == "L" else gR):
                            continue
                        for q in range(ns):
                            out["funccount"] += int(inb[c + q])
                            if above(val[c + q], y):
                                kL, kR = (kL + 1, kR) if side == "L" else (kL, kR + 1)
                            else:
                                if side == "L":
                                    gL = False
                                else:
                                    gR = False
                                break
                        c += ns
                    steps += ns
                Lq, Rq = L0 - float(kL), R0 + float(kR)
                shr = 0
                done = False
                while shr < max_shrink and not done:
                    ns = min(spec, max_shrink - shr)
                    ts = []
                    l_, r_ = Lq, Rq
                    for q in range(ns):
                        t = u[4 + shr + q] * (r_ - l_) + l_
                        ts.append(t)
                        if t < 0.0:
                            l_ = t
                        else:
                            r_ = t
                    P = np.stack([xc + t * v for t in ts])
                    val, inb = values(P, e)
                    out["performed"] += int(np.sum(inb))
                    for q in range(ns):
                        out["funccount"] += int(inb[q])
                        if above(val[q], y):
                            x[e, mine[j]] = P[q]
                            lp[mine[j]] = val[q]
                            done = True
                            break
                        if ts[q] < 0.0:
                            Lq = ts[q]
                        else:
                            Rq = ts[q]
                    shr += ns
            for j in range(H):                     # the record rule of ensemble_slice_sample (vbmc_amd/ensemble.py)
                moved += 1
                if moved > burnin and (moved - burnin) % thin == 0 and nrec < Nm:
                    out["Xa"][nrec, :, e] = x[e, mine[j]]
                    out["logp"][e, nrec] = lp[mine[j]]
                    nrec += 1
            m += 1
        out["halfmoves"] = max(out["halfmoves"], m)
    return out


def halfmoves_needed(Nm, H, thin=1, burnin=None):
    burnin = int(math.ceil(thin * Nm / 2)) if burnin is None else int(burnin)
    return -(-(burnin + Nm * thin) // H)


# name: (D, N, S, W, Nm, thin, meanfun, noisy, low_noise, tight, seed)
CASES = {
    "A": (2, 33, 2, 6, 12, 1, 0, False, False, False, 1),
    "B": (5, 150, 3, 12, 16, 2, 4, True, False, False, 1),
    "C": (3, 40, 2, 8, 10, 1, 1, False, True, False, 1),
    "D": (32, 40, 1, 66, 8, 1, 4, False, False, False, 1),
    "E": (2, 20, 1, 4, 6, 3, 0, False, False, True, 1),
    "F": (3, 530, 1, 6, 6, 1, 1, False, False, False, 1),
}


EDGE_CASES = {
    "G": (2, 16, 1, 6, 6, 1, 0, False, False, False, 1),
    "H": (3, 129, 2, 8, 8, 1, 1, False, True, False, 1),
    "J": (3, 257, 2, 8, 8, 1, 4, False, True, False, 1),
    "T": (3, 1136, 2, 8, 6, 1, 1, False, True, False, 1),
}


def build_case(name):
    from tests._cases import synth_problem

    D, N, S, W, Nm, thin, meanfun, noisy, low_noise, tight, seed = CASES[name] if name in CASES else EDGE_CASES[name]
    p = synth_problem(seed, D, N, 3, S, meanfun=meanfun, noisy=noisy)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(0.03)
    if low_noise:                                  # the hyper-sample S // 2 on the Lchol = false branch (tests/_quad_ref.py::mixed_gp)
        hyp[D + 1, S // 2] = math.log(3e-4)
        hyp[:D, S // 2] += math.log(0.25)
    gp = R.gplite_post(hyp, p["X"], p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    X = gp["X"]
    rng = np.random.default_rng(seed + 900)
    if tight:                                      # a box barely wider than the walkers' spread: stepping out leaves it
        xm = X[int(np.argmax(gp["y"]))]
        LB, UB = xm - 0.15, xm + 0.15
        x0 = xm[None, None, :] + 0.1 * (2 * rng.random((S, W, D)) - 1)
    else:
        diam = np.max(X, axis=0) - np.min(X, axis=0)
        LB, UB = np.min(X, axis=0) - 0.5 * diam, np.max(X, axis=0) + 0.5 * diam
        best = X[np.argsort(-gp["y"], kind="stable")[: max(4, N // 4)]]
        x0 = best[rng.integers(0, best.shape[0], size=(S, W))] + 0.05 * rng.standard_normal((S, W, D))
        x0 = np.minimum(np.maximum(x0, LB), UB)
    H = W // 2
    M = halfmoves_needed(Nm, H, thin)
    U = rng.random((SLOTS, H, S, M + 1))
    U = np.minimum(np.maximum(U, 2.0 ** -53), 1.0 - 2.0 ** -53)
    return {"name": name, "gp": gp, "x0": x0, "LB": LB, "UB": UB, "U": U, "D": D, "N": N, "S": S, "W": W, "H": H, "Nm": Nm, "thin": thin, "M": M}


def oracle_target(gp):
    """logp(P, e): the log base density of acqimiqr_vbmc from the oracle's gplite_pred, hyper-sample e alone (ymu, ys2: the noisy pair)."""

    def logp(P, e):
        ymu, ys2, _, _ = R.gplite_pred(gp, P, None, None, True)
        ymu = np.asarray(ymu).reshape(P.shape[0], -1)[:, e]
        ys = np.sqrt(np.maximum(np.asarray(ys2).reshape(P.shape[0], -1)[:, e], np.finfo(np.float64).tiny))
        return ymu + U_IQR * ys + np.log1p(-np.exp(-2 * U_IQR * ys))

    return logp


_RUNS = {}


def run_case(name):
    """the case and the restatement's answer on the oracle's target, computed once per process and left unchanged"""
    if name not in _RUNS:
        c = build_case(name)
        _RUNS[name] = (c, sample(oracle_target(c["gp"]), c["x0"], c["LB"], c["UB"], c["Nm"], c["U"], thin=c["thin"]))
    return _RUNS[name]

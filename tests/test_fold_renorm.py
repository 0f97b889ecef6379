"""The entropy kernel's running product of mantissas (vbmc_amd/csrc/entropy_mfma.h: fold): sum_i log q'_i is kept as a product of
mantissas pm and a sum of exponents pe, and pm is renormalised every 256 factors.  Renormalising after EVERY factor instead -- the form
measured in profiles/r08_logjoint_rows.md -- goes through the same sequence of mantissas: scaling a double by a power of two is exact
(no underflow: 0.5^256 = 8.6e-78), so only the split of the exponent between pm and pe moves.  Equal mantissa and equal total exponent
at the end, bit for bit, over 200 seeded sequences of 1..5000 factors between e^-600 and e^600.  No GPU."""
import math

import numpy as np


def product(qs, every):
    pm, pe, cnt = 1.0, 0, 0
    for q in qs:
        m, e = math.frexp(q)
        pm *= m
        pe += e
        cnt += 1
        if cnt == every:
            m, e = math.frexp(pm)
            pm, pe, cnt = m, pe + e, 0
    m, e = math.frexp(pm)
    return m, pe + e


def test_renormalising_every_step_equals_every_256():
    rng = np.random.default_rng(20240)
    for _ in range(200):
        n = int(rng.integers(1, 5001))
        qs = np.exp(rng.uniform(-600.0, 600.0, n))
        a, b = product(qs, 1), product(qs, 256)
        assert a[0].hex() == b[0].hex() and a[1] == b[1], (n, a, b)

"""Inputs of the tests of include/vnet_hip_prepare.h (tests/test_prepare_host.py, tests/test_hip_prepare.py, tests/test_hip_prepare_guard.py).

tier E: integer-valued float32 in pairs m +- d around one integer m per channel (plus one m for an odd count), |m|, |d| <= 1024.  The
mean is m, every value, every deviation and every square is an integer, and for n <= 2^21: sum |x| <= 2^21 * 2^11 = 2^32 and
sum d^2 <= 2^21 * 2^20 = 2^41, far below 2^53 -- every partial sum in fp64 is exact IN ANY ORDER, so sum, css, min and max of two correct
implementations are equal bit for bit.
tier B: N(40, 300) float32 with |x| >= 1 forced: one dropped or doubled element moves the sum by at least 1, orders of magnitude above the
worst-case rounding bound (n - 1) * 2^-53 * sum |x| of any summation order."""
import math

import numpy as np


def tier_e(n, C, seed=0):
    rng = np.random.default_rng([seed, n, C])
    out = np.empty((n, C), np.float32)
    for c in range(C):
        m = int(rng.integers(-1024, 1025))
        d = rng.integers(0, 1025, size=n // 2)
        col = np.concatenate([m + d, m - d, [m] * (n % 2)]).astype(np.float64)
        out[:, c] = rng.permutation(col)
    return out


def tier_b(n, C, seed=0):
    x = np.random.default_rng([seed, n, C, 7]).normal(40.0, 300.0, (n, C)).astype(np.float32)
    return np.where(np.abs(x) < 1.0, np.float32(1.0), x).astype(np.float32)


def fsum_stats(x, pre=None, mean=None):
    """float64 [C, 4] = {sum, css, min, max} with math.fsum (exactly rounded sums) of v = (x - a) / b formed in double; css about
    `mean` ([C]; None: about fsum / n)."""
    n, C = x.shape
    out = np.empty((C, 4), np.float64)
    for c in range(C):
        v = x[:, c].astype(np.float64)
        if pre is not None:
            v = (v - pre[c][0]) / pre[c][1]
        s = math.fsum(v)
        m = np.float64(s) / np.float64(n) if mean is None else np.float64(mean[c])
        out[c] = s, math.fsum((v - m) ** 2), v.min(), v.max()
    return out

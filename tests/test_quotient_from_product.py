"""The quotient-from-product modular multiply (csrc/kernels.h fmul_remq), restated in NumPy float64
and checked against Python integers.

    p = a*w;  pl = fma(a, w, -p);  qh = rint(p * qi);  u = fma(-qh, q, p);  r = u + pl

NumPy has no fma: each fma is modelled as its exact integer result, and the test asserts that this
result is representable in a double -- the property the device code relies on (a representable
exact value is what the single rounding of an fma returns).  Checked for every prime of the bench
chain (N = 2^16, L = 30, K = 10, scale 40: the 40-bit class, the 50-bit q_0 and special primes) and
of a scale-42 chain whose primes lie on either side of the 2^42 split, as the oracle reports them:

* p - qh*q and a*w - p are exactly representable, and so is their sum r;
* r is congruent to a*w mod q;
* |r| <= (1/2 + eps) q with eps = 3 * 2^-53 * |a*w/q| * (1 + 2^-52), the bound documented beside
  fmul_remq (p, qi and p * qi carry one rounding each); for |a| < 2^51 that is below 1.25q, and
  below q while |a*w/q| < 2^53 / 6.

The last test takes the quotient with a qi that is one ulp further from 1/q than its rounding
and asserts that the same check then fails: the bound has no slack for a wrong qi.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from aes_xor_fhe._abi import Params

AMAX = (1 << 51) - 1
RANDOM_PAIRS = 1500  # per prime, beside the 11 x 5 edge pairs


def _chain(lib, log_n, max_level, special_primes, scale_bits):
    cp = Params(log_n, max_level, special_primes, scale_bits, 50, 50, 0, 0, 0, None)
    primes = (C.c_uint64 * (max_level + 1 + special_primes))()
    scales = (C.c_double * (max_level + 1))()
    lib.check(lib.chain(C.byref(cp), primes, scales))
    return [int(q) for q in primes]


def _exact(x):
    """x (object array of Python integers) -> True where float64 holds it exactly."""
    return np.array([int(float(v)) == v for v in x], dtype=bool)


def fmul_remq_checked(a, w, q, qi):
    """The primitive on integer arrays a, w (object dtype) for one prime: (r, failures), r the
    exact integers the device code returns, failures a list of (property, index)."""
    af, wf = a.astype(np.float64), w.astype(np.float64)
    assert _exact(a).all() and _exact(w).all()
    aw = a * w                                   # exact (Python integers)
    p = af * wf                                  # one rounding
    pi = np.array([int(v) for v in p], dtype=object)
    pl = aw - pi                                 # fma(a, w, -p): exact if representable
    qh = np.rint(p * qi)
    qhi = np.array([int(v) for v in qh], dtype=object)
    u = pi - qhi * q                             # fma(-qh, q, p)
    r = u + pl
    fails = []
    for name, ok in (("a*w - p representable", _exact(pl)), ("p - qh*q representable", _exact(u)),
                     ("r representable", _exact(r)),
                     ("r == a*w mod q", np.array([(x - y) % q == 0 for x, y in zip(r, aw)], dtype=bool)),
                     # |r| <= q/2 + 3 * 2^-53 |a w| (1 + 2^-52), times 2^106
                     ("|r| <= (1/2 + eps) q", np.array([abs(x) << 106 <= (q << 105) + 6 * abs(y) * ((1 << 52) + 1)
                                                        for x, y in zip(r, aw)], dtype=bool))):
        fails += [(name, int(i)) for i in np.flatnonzero(~ok)]
    return r, fails


def _operands(q, rng):
    edge_a = [0, 1, -1, AMAX, -AMAX, q // 2, -(q // 2), 9 * q, -9 * q, 17 * q, -17 * q]
    edge_a = [v for v in edge_a if abs(v) <= AMAX]
    edge_w = [0, 1, q - 1, q // 2, (q + 1) // 2]
    a = [x for x in edge_a for _ in edge_w]
    w = [y for _ in edge_a for y in edge_w]
    # random: |a| up to 2^51 - 1 (half of them within 2^k of the top), w over [0, q)
    ra = rng.integers(-AMAX, AMAX + 1, RANDOM_PAIRS)
    ra[::2] = np.sign(ra[::2]) * (AMAX - rng.integers(0, 1 << 20, len(ra[::2])))
    rw = rng.integers(0, q, RANDOM_PAIRS)
    rw[::4] = q - 1 - rng.integers(0, 1 << 10, len(rw[::4]))
    a += [int(v) for v in ra]
    w += [int(v) for v in rw]
    return np.array(a, dtype=object), np.array(w, dtype=object)


def test_every_bench_prime_and_the_2_42_split(oracle_lib):
    bench = _chain(oracle_lib, 16, 30, 10, 40)
    split = _chain(oracle_lib, 16, 8, 4, 42)
    assert sum(abs(q - (1 << 40)) < 1 << 26 for q in bench) == 30 and sum(q > 1 << 49 for q in bench) == 11
    assert any(q < 1 << 42 for q in split[1:9]) and any(1 << 42 <= q < 1 << 43 for q in split[1:9])
    rng = np.random.default_rng(51)
    worst = Fraction(0)
    for q in sorted(set(bench + split)):
        assert q % 2 == 1 and q < 1 << 50
        a, w = _operands(q, rng)
        r, fails = fmul_remq_checked(a, w, q, 1.0 / float(q))
        assert not fails, f"q = {q}: {fails[:3]} (a, w = {a[fails[0][1]]}, {w[fails[0][1]]})"
        worst = max(worst, max(Fraction(abs(int(x)), q) for x in r))
    # |a| < 2^51: eps < 3/4
    assert Fraction(1, 2) < worst < Fraction(5, 4)


def test_a_wrong_qi_fails_the_bound(oracle_lib):
    """qi one ulp further from 1/q than its correct rounding: the quotient error then exceeds eps
    for operands near the top of the range, and the bound check reports it."""
    q = _chain(oracle_lib, 16, 30, 10, 40)[0]  # the 50-bit q_0: 1/q sits low in its binade, ulp = 2^-52 relative
    qi = 1.0 / float(q)
    err = Fraction(qi) - Fraction(1, q)
    bad_qi = float(np.nextafter(qi, np.inf if err >= 0 else -np.inf))
    assert abs(Fraction(bad_qi) - Fraction(1, q)) > Fraction(1, q) / (1 << 53)  # no longer a correct rounding
    rng = np.random.default_rng(52)
    n = 4000
    a = np.array([AMAX - int(v) for v in rng.integers(0, 1 << 30, n)], dtype=object)
    w = np.array([q - 1 - int(v) for v in rng.integers(0, 1 << 30, n)], dtype=object)
    _, fails = fmul_remq_checked(a, w, q, qi)
    assert not fails
    _, fails = fmul_remq_checked(a, w, q, bad_qi)
    assert fails and {name for name, _ in fails} == {"|r| <= (1/2 + eps) q"}, fails[:3]

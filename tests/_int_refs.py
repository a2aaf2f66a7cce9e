"""Exact references in Python integers for the operations of include/aesfhe.h that have one.

Every function here works on numpy `object` arrays of Python ints (or on plain ints) and states
one operation's arithmetic from its definition, not from either implementation.  The only
compiled code a reference may use is the CPU oracle's ntt_host (pinned to the schoolbook KAT in
test_oracle_ckks.py) to move a limb between coefficient and NTT form: `ntt_limbs`.

A reference takes the rule it could get wrong as a keyword (`ge`: centre with >= instead of >,
`sat`: clamp to +-(2^63 - 1), `half_even`: the rounding of ties), so that the tests can show that
the comparison they make would fail under the other rule (tests/test_integer_witnesses.py)."""
import ctypes as C
from fractions import Fraction

import numpy as np

I64_MAX = (1 << 63) - 1


def obj(a):
    """Any integer array as Python ints."""
    return np.asarray(a).astype(object)


def u64(a):
    return np.array(a, dtype=np.uint64)


def ntt_limbs(eng, limbs, pids, inverse):
    """(nlimb, n) words through eng's ntt_host, limb r with prime index pids[r]: a copy."""
    buf = np.ascontiguousarray(limbs, dtype=np.uint64).copy()
    assert buf.ndim == 2 and len(pids) == buf.shape[0]
    p = np.asarray(pids, dtype=np.int32)
    eng._check(eng._lib.ntt_host(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.shape[0],
                                 p.ctypes.data_as(C.POINTER(C.c_int32)), inverse))
    return buf


def ntt_poly(eng, x, inverse):
    """(..., nl, n) residues whose axis -2 is limbs 0..nl-1: every limb transformed."""
    x = np.asarray(x, dtype=np.uint64)
    nl, n = x.shape[-2:]
    flat = x.reshape(-1, n)
    return ntt_limbs(eng, flat, np.arange(flat.shape[0]) % nl, inverse).reshape(x.shape)


# ------------------------------------------------------------------------------------------------
def tensor_ref(a, b, primes):
    """(a0 b0, a0 b1 + a1 b0, a1 b1) mod q per limb in Python integers: (B, 3, l + 1, n)."""
    ao, bo = a.astype(object), b.astype(object)
    out = np.empty((a.shape[0], 3) + a.shape[2:], dtype=np.uint64)
    for i in range(a.shape[2]):
        q = primes[i]
        out[:, 0, i] = (ao[:, 0, i] * bo[:, 0, i]) % q
        out[:, 1, i] = (ao[:, 0, i] * bo[:, 1, i] + ao[:, 1, i] * bo[:, 0, i]) % q
        out[:, 2, i] = (ao[:, 1, i] * bo[:, 1, i]) % q
    return out


def residues_ref(x, primes):
    """Signed integers (..., n) -> their residues in [0, q): (..., len(primes), n)."""
    xo = obj(x)
    return u64(np.stack([xo % q for q in primes], axis=-2))


def centre(v, m, ge=False):
    """v in [0, m) -> (-m/2, m/2]: v - m if v > m // 2 (ge: if v >= m // 2, the wrong rule)."""
    v = obj(v)
    return np.where((v >= m // 2) if ge else (v > m // 2), v - m, v)


def crt2(r0, r1, q0, q1):
    """The x in [0, q0 q1) with x = r0 mod q0 and x = r1 mod q1 (the symmetric CRT formula)."""
    return (obj(r0) * (q1 * pow(q1, -1, q0)) + obj(r1) * (q0 * pow(q0, -1, q1))) % (q0 * q1)


def decrypt_ref(x, Q, ge=False, sat=True):
    """aesfhe_decrypt of an encryption of the integers x: sat(centre(x mod Q)) as int64 (sat=False:
    the low 64 bits, as a conversion without the clamp would give)."""
    c = centre(obj(x) % Q, Q, ge)
    if sat:
        c = np.where(c > I64_MAX, I64_MAX, np.where(c < -I64_MAX, -I64_MAX, c))
    else:
        c = (c + (1 << 63)) % (1 << 64) - (1 << 63)
    return np.array(c, dtype=np.int64)


def lift_ref(v, q0, q, ge=False):
    """ModRaise of one coefficient-form limb: centre_{q0}(v) mod q."""
    return u64(centre(v, q0, ge) % q)


def mul_i_ref(x, q, sign):
    """Coefficient form (..., n) times X^{n/2} (sign > 0) or -X^{n/2} in Z_q[X] / (X^n + 1)."""
    x = obj(x)
    h = x.shape[-1] // 2
    out = np.empty_like(x)
    out[..., h:] = x[..., :h]
    out[..., :h] = (-x[..., h:]) % q
    return u64(out if sign > 0 else (-out) % q)


def galois_ref(x, g, q):
    """Coefficient form (..., n) under X -> X^g: coefficient k moves to g k mod 2n, negated when
    that is >= n."""
    x = obj(x)
    n = x.shape[-1]
    t = (g * np.arange(n, dtype=np.int64).astype(object)) % (2 * n)
    idx = np.array(t % n, dtype=np.int64)
    assert len(set(idx.tolist())) == n
    neg = np.array(t >= n, dtype=bool)
    out = np.empty_like(x)
    out[..., idx] = np.where(neg, (-x) % q, x)
    return u64(out)


def level_down_const_ref(scales, primes, l):
    """The constant of the exact-scale level-down l -> l - 1: floor(D_{l-1} q_l / D_l + 0.5)."""
    import math
    return int(math.floor(scales[l - 1] * float(primes[l]) / scales[l] + 0.5))


def rescale_ref(oracle, x, primes, C=1, ge=False):
    """Rescale of C x for x of shape (..., l + 1, n) in NTT form: limb i < l of the result is
    (C x_i - NTT_i(centre_{q_l}(C x_l))) q_l^{-1} mod q_i, the top limb taken in coefficient form."""
    x = np.asarray(x, dtype=np.uint64)
    l, n = x.shape[-2] - 1, x.shape[-1]
    ql = primes[l]
    top = ntt_limbs(oracle, x[..., l, :].reshape(-1, n), [l] * (x.size // ((l + 1) * n)), 1).reshape(x[..., l, :].shape)
    v = centre((C * obj(top)) % ql, ql, ge)
    out = np.empty(x.shape[:-2] + (l, n), dtype=np.uint64)
    for i in range(l):
        q = primes[i]
        t = ntt_limbs(oracle, u64(v % q).reshape(-1, n), [i] * (v.size // n), 0).reshape(v.shape)
        out[..., i, :] = u64(((C * obj(x[..., i, :]) - obj(t)) * pow(ql, -1, q)) % q)
    return out


def dot_pt_sum_ref(cts, pts, primes):
    """sum_i ct_i pt_i mod q, before the rescale: cts[i] (B, np, l + 1, n), pts[i] (l + 1, n).
    Equal (ct, pt) pairs (by identity) are multiplied once and counted."""
    pairs = {}
    for c, p in zip(cts, pts):
        k = (id(c), id(p))
        pairs[k] = (c, p, pairs.get(k, (c, p, 0))[2] + 1)
    acc = None
    for c, p, cnt in pairs.values():
        t = obj(c) * obj(p)[None, None] * cnt
        acc = t if acc is None else acc + t
    out = np.empty(acc.shape, dtype=np.uint64)
    for i in range(acc.shape[2]):
        out[:, :, i] = u64(acc[:, :, i] % primes[i])
    return out


def round_tie(c, half_even=False):
    """The integer nearest to the double c, ties away from zero (half_even: to even)."""
    if half_even:
        return round(Fraction(c))
    f = Fraction(c)
    m = (abs(f) + Fraction(1, 2)).__floor__()
    return m if f >= 0 else -m

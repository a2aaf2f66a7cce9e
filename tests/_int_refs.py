"""Exact references in Python integers for the operations of include/aesfhe.h that have one.

Every function here works on numpy `object` arrays of Python ints (or on plain ints) and states
one operation's arithmetic from its definition, not from either implementation.  The only
compiled code a reference may use is the CPU oracle's ntt_host (pinned to the schoolbook KAT in
test_oracle_ckks.py) to move a limb between coefficient and NTT form: `ntt_limbs`.

A reference takes the rule it could get wrong as a keyword (`ge`: centre with >= instead of >,
`sat`: clamp to +-(2^63 - 1), `half_even`: the rounding of ties), so that the tests can show that
the comparison they make would fail under the other rule (tests/test_integer_witnesses.py,
tests/test_keyswitch_witness.py: `floor`, `exact`, `every_limb`)."""
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


# ------------------------------------------------------------------------------------------------
# the hybrid key switch
def _ntt(eng, limbs, pids, inverse):
    """(..., len(pids), n) words, limb r of axis -2 with prime index pids[r]; eng is an engine (its
    ntt_host) or any callable (limbs (m, n), pids (m), inverse) -> (m, n) (the hand case)."""
    x = np.asarray(limbs, dtype=np.uint64)
    n = x.shape[-1]
    flat = x.reshape(-1, n)
    p = [pids[i % len(pids)] for i in range(flat.shape[0])]
    out = eng(flat, p, inverse) if callable(eng) else ntt_limbs(eng, flat, p, inverse)
    return np.asarray(out, dtype=np.uint64).reshape(x.shape)


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def ks_pids(l, L, K):
    """Prime indices of the l + 1 + K limbs of Q_l u P: q_0..q_l, then p_0..p_{K-1} (stored after
    all L + 1 primes of Q)."""
    return list(range(l + 1)) + [L + 1 + k for k in range(K)]


def modup_ref(coef_digit, digit_primes, target_primes, exact=False):
    """The approximate base conversion of one digit: coef_digit (..., alpha, n) in coefficient
    form, y_i = [x_i (Q_d / q_i)^{-1}]_{q_i}, S = sum_i y_i (Q_d / q_i) as an integer that is not
    reduced mod Q_d (its overshoot u Q_d, 0 <= u < alpha, is part of the definition); the result
    is S mod p for every target p: (..., len(target_primes), n).  A target inside the digit gets
    x_i back.  exact: S mod Q_d first, the conversion the engine does not do (the wrong rule)."""
    x = obj(coef_digit)
    Qd = _prod(digit_primes)
    S = 0
    for i, q in enumerate(digit_primes):
        hat = Qd // q
        S = S + ((x[..., i, :] * pow(hat, -1, q)) % q) * hat
    if exact:
        S = S % Qd
    return u64(np.stack([S % p for p in target_primes], axis=-2))


def ks_acc_ref(eng, d, l, key, A, primes, K, exact=False):
    """The key switch's inner product over Q_l u P: d (..., l + 1, n) in NTT form, key the
    residues of aesfhe_key_export (digits, 2: b then a, L + 1 + K, n).  For digit j,
    ext_j = NTT(modup_ref(INTT(d) on the digit's limbs)) on all l + 1 + K limbs, and
    acc[c, t] = sum_j ext_j[t] key[j, c, pid(t)] mod p_t: (..., 2, l + 1 + K, n) Python ints."""
    L = len(primes) - 1 - K
    pids = ks_pids(l, L, K)
    tp = [primes[p] for p in pids]
    dc = _ntt(eng, d, list(range(l + 1)), 1)
    key = np.asarray(key)
    acc = None
    for j, lo in enumerate(range(0, l + 1, A)):
        hi = min(lo + A, l + 1)
        ext = obj(_ntt(eng, modup_ref(dc[..., lo:hi, :], primes[lo:hi], tp, exact), pids, 0))
        t = ext[..., None, :, :] * obj(key[j][:, pids])
        acc = t if acc is None else acc + t
    for t, p in enumerate(tp):
        acc[..., t, :] %= p
    return acc


def moddown_ref(eng, acc, l, r, primes, K, margin_bits=40, floor=False):
    """ModDown of acc (..., l + 1 + K, n; NTT form) by D = the product of the dropped limbs
    E = {q_{l-r+1}..q_l, p_0..p_{K-1}}: X in [0, D) is the CRT of E's limbs in coefficient form,
    conv = X - D [2 X > D] (the centred remainder: the division rounds to nearest; D is odd, so
    there is no tie), out_i = (acc_i - NTT_i(conv mod q_i)) D^{-1} mod q_i for i <= l - r.
    floor: conv = X (the wrong rule: the division rounds down).
    Returns (out (..., l - r + 1, n) uint64, ambiguous (..., n) bool): ambiguous are the
    coefficients with |X / D - 1/2| <= 2^-margin_bits, where an fp64 sum of the y_j / e_j (error
    below 2^-43) may round either way."""
    L = len(primes) - 1 - K
    pids = ks_pids(l, L, K)
    lk = l - r
    E = [primes[p] for p in pids[lk + 1:]]
    D = _prod(E)
    a = np.asarray(acc)
    co = obj(_ntt(eng, u64(a[..., lk + 1:, :]), pids[lk + 1:], 1))
    X = 0
    for j, ej in enumerate(E):
        hat = D // ej
        X = X + co[..., j, :] * (hat * pow(hat, -1, ej))
    X = X % D
    up = np.array(2 * X > D, dtype=bool)
    conv = X if floor else X - D * up.astype(object)
    amb = np.array(abs(2 * X - D) * (1 << (margin_bits - 1)) <= D, dtype=bool)
    cv = _ntt(eng, u64(np.stack([conv % primes[i] for i in range(lk + 1)], axis=-2)), list(range(lk + 1)), 0)
    out = np.empty(a.shape[:-2] + (lk + 1, a.shape[-1]), dtype=np.uint64)
    for i in range(lk + 1):
        q = primes[i]
        out[..., i, :] = u64(((obj(a[..., i, :]) - obj(cv[..., i, :])) * pow(D, -1, q)) % q)
    return out, amb


def keyswitch_ref(eng, d, l, key, A, primes, K, r=0, addend=None, exact=False, floor=False):
    """Key switch of d (..., l + 1, n) combined with r rescales: ks_acc_ref, then (r >= 1) P times
    addend (..., 2, l + 1, n) added on the Q limbs, then moddown_ref: (out (..., 2, l - r + 1, n),
    ambiguous (..., 2, n))."""
    acc = ks_acc_ref(eng, d, l, key, A, primes, K, exact)
    if addend is not None:
        P = _prod(primes[len(primes) - K:])
        for i in range(l + 1):
            acc[..., i, :] = (acc[..., i, :] + P * obj(addend[..., i, :])) % primes[i]
    return moddown_ref(eng, acc, l, r, primes, K, floor=floor)


def ksk_error_ref(eng, key, s, s_prime, A, primes, K, every_limb=False):
    """The error polynomial of a switching key from s' to s: for digit j and limb p
    of Q u P, b + a s - [p in digit j] P s' mod p in coefficient form, centred: (digits, L + 1 + K,
    n) Python ints.  key, s, s_prime are NTT-form residues (key as ks_acc_ref's).  For a good key
    it is the same small polynomial on every limb.  every_limb: P s' on every limb of Q (wrong)."""
    np_ = len(primes)
    L = np_ - 1 - K
    P = _prod(primes[L + 1:])
    key = np.asarray(key)
    out = []
    for j in range(key.shape[0]):
        lo, hi = j * A, min(j * A + A, L + 1)
        v = []
        for p, q in enumerate(primes):
            t = obj(key[j, 0, p]) + obj(key[j, 1, p]) * obj(s[p])
            if lo <= p < hi or (every_limb and p <= L):
                t = t - P * obj(s_prime[p])
            v.append(t % q)
        co = obj(_ntt(eng, u64(np.stack(v)), list(range(np_)), 1))
        out.append(np.stack([centre(co[p], q) for p, q in enumerate(primes)]))
    return np.stack(out)

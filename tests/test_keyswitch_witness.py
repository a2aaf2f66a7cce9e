"""The hybrid key switch against references in Python integers: ModUp, the switching keys, ModDown
at its ties.

The other key-switch suites (test_keyswitch_shapes.py, test_range_bounds.py, test_gpu_parity.py)
compare the HIP engine with the CPU oracle, and the oracle's own key switch is checked through
noise-tolerant decryptions only.  Here the key switch has a third witness (_int_refs.py: modup_ref,
ks_acc_ref, moddown_ref, keyswitch_ref, ksk_error_ref), stated from DESIGN.md 3.7 / 3.12 and not
from either implementation, with the oracle's ntt_host as the only compiled ingredient.

  A  real keys (relinearisation, fixed rotation, hoisted rotation; read with key_export), seeded
     random residues: relinearize (r = 0), multiply (r = 1), poly2_int (r = 2), rotate,
     rotate_hoisted, and the key identity b + a s - [limb in digit] P s' = e with one small e
     (|e| <= 21, the range of cbd21) on every limb of Q u P.
  B  constructed accumulators: a key imported residue by residue whose digit 0 alone is non-zero,
     and d = 1 on digit 0, make acc = W, an integer per coefficient that the test chooses: eight
     equal runs, four within 2^-40 of a ModDown tie (next to it and D >> 60 away), two just
     outside the margin (D >> 38 away), v = 0 and v = K + r (every y_j = e_j - 1); in the second
     component every coefficient of the runs near the tie has source words of its own.

ModDown's exact conversion takes v = rint(sum_j y_j (1 / e_j)) in fp64; within 2^-40 of a tie
(moddown_ref's `ambiguous` mask; the margin is derived in DESIGN.md 3.12) fp64 may round either
way.  Section A asserts that no coefficient of its inputs is ambiguous (a condition on the seeds,
not a tolerance) and compares whole arrays; Section B asserts that exactly its four tie runs are
ambiguous, that each of those coefficients is floor(W / D) or floor(W / D) + 1 with the same choice
on every limb, and that everything else equals the reference.  HIP engine against oracle is
np.array_equal over everything, the ambiguous coefficients included (the oracle's
sum is the contract).

Every `_check_*` takes (e, o) as in test_integer_witnesses.py: the CPU tests run it with e = o at
N = 2^12 and show that the comparison bites; the GPU tests run it through `_both`.  A reference is
computed once per pair of engines (`cache`), after checking that both hold the same key words.
Each check prints its figures (wall time, ambiguous coefficients, how many of them rounded up and
down): run with -s to see them."""
import time

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine, RelinearizationKey

from _int_refs import (_ntt, galois_ref, keyswitch_ref, ks_acc_ref, ks_pids, ksk_error_ref, moddown_ref,  # noqa: E402
                       modup_ref, ntt_poly, obj, round_tie, tensor_ref, u64)
from _ks_helpers import (N16, _check_path, _drop, _key_from_residues, _key_residues, _pair, _pool,  # noqa: E402
                         _profiled, ks_plan)
from test_integer_witnesses import W12, W16, W17, _both, _eq, _n, _secret_residues  # noqa: E402

K16 = dict(log_n=12, max_level=17, special_primes=16, digit_primes=16, scale_bits=40, seed=31)
K15 = dict(log_n=12, max_level=16, special_primes=15, digit_primes=15, scale_bits=40, seed=32)
WIDE16 = dict(log_n=16, max_level=13, special_primes=12, digit_primes=12, scale_bits=40, seed=33)
OPS = ("relinearize", "multiply", "poly2_int", "rotate", "rotate_hoisted")
RESCALES = dict(relinearize=0, multiply=1, poly2_int=2, rotate=0, rotate_hoisted=0)
POLY2_W, POLY2_DEN = 5, 64
HOIST_DELTAS = (-1, 5)
ERR_MAX = 21  # cbd21


def _report(what, t0, **figures):
    print(f"[keyswitch-witness] {what}: {time.time() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()))


def _kap(e):
    return e.special_prime_count, e.digit_primes, e.primes


class _Keys:
    """One secret key and, made on first use, the switching keys with their exported residues."""

    def __init__(self, e):
        self.e, self.sk, self._k = e, e.create_secret_key(9), {}

    def get(self, name):
        if name not in self._k:
            e, sk = self.e, self.sk
            if name == "rlk":
                key = e.create_relinearization_key(sk)
            elif name == "rot":
                key = e.create_fixed_rotation_key(sk, 1)
            else:
                key = e.create_hoisted_rotation_key(sk, HOIST_DELTAS[int(name[1:])])
            kind, g, res = _key_residues(e, key)
            assert kind == dict(r=2 if name == "rlk" else 3, h=5)[name[0]] and res.shape[0] == e.dnum
            self._k[name] = (key, g, res)
        return self._k[name]


def _keys(e):
    if getattr(e, "_witness_keys", None) is None:
        e._witness_keys = _Keys(e)
    return e._witness_keys


def _release(*engines):
    for e in engines:
        e._witness_keys = None
    _drop(*engines)


def _run(e, o, l, op, what, fn):
    """fn() on e; on the HIP engine with the launch profile read: at N = 2^16 compared with ks_plan
    (which kernels ran, not only that some path gave the right residues), at the other sizes the
    unfused conversion (engine.hip moddown_conv: k_bconv_mfma<., true> while K + r + 1 <= 16,
    k_moddown<K + r> above) must have run and the column-fused one must not."""
    if e._lib is o._lib:
        return fn()
    K, A, _ = _kap(e)
    res, prof = _profiled(e, fn)
    if _n(e) == N16:
        _check_path(prof, K, A, l, op, what)
    else:
        nks = len(HOIST_DELTAS) if op == "rotate_hoisted" else 1
        assert prof.get("moddown", 0) == nks and not prof.get("moddown_cols", 0), f"{what}: launches {prof}"
    return res


def _ks_ref(e, o, cache, tag, d, l, key, r=0, addend=None):
    """keyswitch_ref of d with `key`, once per pair of engines; no coefficient may be ambiguous."""
    k = (tag, l, r)
    if k not in cache:
        K, A, primes = _kap(e)
        t0 = time.time()
        out, amb = keyswitch_ref(o, d, l, key, A, primes, K, r, addend)
        _report(f"reference {tag}, N = {_n(e)}, K = {K}, level {l}, r = {r}", t0, ambiguous=int(amb.sum()))
        cache[k] = (key, d, out, amb)
    key0, d0, out, amb = cache[k]
    assert (key0 is key or np.array_equal(key0, key)) and (d0 is d or np.array_equal(d0, d)), \
        f"{tag}: the engines of a pair differ in the key or the input"
    assert not amb.any(), f"{tag} at level {l}: {int(amb.sum())} coefficients within 2^-40 of a ModDown tie; " \
                          f"choose another seed"
    return out


def _addq(a, b, q):
    """a + b mod q per limb: (..., len(q), n)."""
    return u64(np.stack([(obj(a[..., i, :]) + obj(b[..., i, :])) % p for i, p in enumerate(q)], axis=-2))


def _sigma(o, x, g, q):
    """NTT-form limbs (..., len(q), n) of Q under X -> X^g, through coefficient form."""
    co = ntt_poly(o, x, 1)
    return ntt_poly(o, np.stack([galois_ref(co[..., i, :], g, p) for i, p in enumerate(q)], axis=-2), 0)


# ------------------------------------------------------------------------------------------------
# Section A: real keys, random residues
def _check_ops(e, o, l, ops=OPS, seed=4100, cache=None):
    cache = {} if cache is None else cache
    n = _n(e)
    B = 2 if n <= 1 << 12 else 1
    K, A, primes = _kap(e)
    q = primes[:l + 1]
    pool = _pool(primes, l, B, 6, seed + l, n=n)
    imp = lambda a: e.import_residues(np.ascontiguousarray(a))  # noqa: E731
    ks = _keys(e)
    outs = []
    for op in ops:
        t0 = time.time()
        r = RESCALES[op]
        what = f"{op} at N = {n}, K = {K}, A = {A}, level {l}"
        if op == "relinearize":
            key, _, kr = ks.get("rlk")
            arr = pool[:, 3:6]
            want = [_addq(_ks_ref(e, o, cache, op, arr[:, 2], l, kr), arr[:, :2], q)]
            got = _run(e, o, l, op, what, lambda: [e.relinearize(imp(arr), key)])
        elif op in ("multiply", "poly2_int"):
            key, _, kr = ks.get("rlk")
            x, y = pool[:, 0:2], pool[:, 2:4]
            t = tensor_ref(x, y, q)
            if op == "poly2_int":  # F = w llround(S1 / den) mod q, the floats in the header's order
                D = e.scales
                S1 = D[l - 2] / D[l] * (float(primes[l]) / D[l]) * float(primes[l - 1])
                H = round_tie(S1 / float(POLY2_DEN))
                assert H > 1
                t = u64(np.stack([(obj(t[:, :, i]) * ((POLY2_W * H) % p)) % p for i, p in enumerate(q)], axis=2))
            want = [_ks_ref(e, o, cache, op, t[:, 2], l, kr, r=r, addend=t[:, :2])]

            def fn():
                if op == "poly2_int":
                    return e.poly2_int([imp(x)], [imp(y)], [[0, 0], [0, POLY2_W]], POLY2_DEN, key)
                out = e.multiply(imp(x), imp(y), key)
                out._h  # the product is deferred: evaluate it here
                return [out]
            got = _run(e, o, l, op, what, fn)
        elif op == "rotate":
            key, g, kr = ks.get("rot")
            ct = pool[:, 4:6]
            p = _sigma(o, ct, g, q)
            k = _ks_ref(e, o, cache, op, p[:, 1], l, kr)
            want = [np.stack([_addq(p[:, 0], k[:, 0], q), k[:, 1]], axis=1)]
            got = _run(e, o, l, op, what, lambda: [e.rotate(imp(ct), key)])
        else:
            hk = [ks.get(f"h{i}") for i in range(len(HOIST_DELTAS))]
            ct = pool[:, 1:3]
            want = []
            for i, (_, g, kr) in enumerate(hk):
                k = _ks_ref(e, o, cache, f"{op}[{i}]", ct[:, 1], l, kr)
                want.append(_sigma(o, np.stack([_addq(ct[:, 0], k[:, 0], q), k[:, 1]], axis=1), g, q))
            got = _run(e, o, l, op, what, lambda: e.rotate_hoisted(imp(ct), [h[0] for h in hk]))
        assert len(got) == len(want)
        for i, (c, w) in enumerate(zip(got, want)):
            assert (c.level, c.batch, c.npoly, c.is_zero) == (l - r, B, 2, False), f"{what}: {c!r}"
            a = e.export_residues(c)
            _eq(a, w, f"{what}, output {i}, against the integers")
            outs.append(a)
        _report(what, t0, ambiguous=0)
    return outs


def _key_cases(e, o):
    """(name, key residues, s, s') of the three kinds: the key switches from s' to s."""
    ks = _keys(e)
    primes = e.primes
    s = _secret_residues(e, ks.sk)
    every = lambda g: _sigma(o, s, g, primes)  # noqa: E731  (all limbs of Q u P: prime indices 0..np-1)
    _, _, rl = ks.get("rlk")
    _, g, rot = ks.get("rot")
    _, gh, hoist = ks.get("h0")
    s2 = u64(np.stack([(obj(s[p]) * obj(s[p])) % q for p, q in enumerate(primes)]))
    ginv = pow(gh, -1, 2 * _n(e))
    return [("relinearisation", rl, s, s2), ("rotation", rot, s, every(g)), ("hoisted rotation", hoist, every(ginv), s)]


def _check_key_identity(e, o):
    """b + a s - [limb in digit] P s' is one small polynomial per digit, the same on every limb of
    Q u P: pins k_key_combine and the key layout.  Relinearisation: s' = s^2; rotation by g:
    s' = sigma_g(s); hoisted rotation by g: the key switches from s to sigma_g^{-1}(s)."""
    K, A, primes = _kap(e)
    outs = []
    for name, key, s, sp in _key_cases(e, o):
        t0 = time.time()
        err = ksk_error_ref(o, key, s, sp, A, primes, K)
        assert err.shape[:2] == (e.dnum, len(primes))
        same = err == err[:, :1]
        assert same.all(), f"{name} key: the error differs between limbs at [digit, limb, coeff] = " \
                           f"{np.argwhere(~same)[0].tolist()}"
        m = max(abs(int(v)) for v in err[:, 0].ravel())
        assert 0 < m <= ERR_MAX, f"{name} key: max |e| = {m}"
        assert all((err[j, 0] != err[0, 0]).any() for j in range(1, e.dnum)), f"{name} key: digits share an error"
        outs.append(np.array(err[:, 0], dtype=np.int64))
        _report(f"{name} key identity at N = {_n(e)}, K = {K}", t0, max_e=m)
    return outs


# ------------------------------------------------------------------------------------------------
# Section B: constructed accumulators
def _crt_from_y(y, E, D):
    """The X in [0, D) whose ModDown source words are y_j: acc_j = y_j (D / e_j) mod e_j."""
    X = 0
    for yj, ej in zip(y, E):
        hat = D // ej
        X += ((yj * hat) % ej) * hat * pow(hat, -1, ej)
    X %= D
    assert all((X * pow(D // ej, -1, ej)) % ej == yj for yj, ej in zip(y, E))
    return X


def _tie_values(E, n, seed):
    """W (2, n) Python ints in eight equal runs and the mask of the four tie runs.  Component 0:
    m D + (D - 1) / 2, m D + (D + 1) / 2 (random m < 2^62), these -+ (D >> 60), (D -+ 1) / 2 -+
    (D >> 38), v = 0, v = K + r.  A run of component 0 has one X = W mod D, so one vector of
    source words y_j and one fp64 sum; component 1 (its runs rotated by three places) therefore
    moves runs 3 to 6 further by a random distance per coefficient, up to D >> 60 inside the margin
    and up to D >> 38 outside it: every coefficient then has its own y_j, all of them with
    sum_j y_j / e_j within 2^-59 of a half-integer (runs 3, 4) or 2^-38 to 2^-37 from it (5, 6)."""
    D = 1
    for ej in E:
        D *= ej
    assert D % 2 == 1 and D >> 60 > 0
    rng = np.random.default_rng(seed)
    w = n // 8
    nb = (D.bit_length() + 7) // 8
    upto = lambda hi: np.array([int.from_bytes(rng.bytes(nb), "little") % (hi + 1) for _ in range(w)], dtype=object)  # noqa: E731
    W, tie = np.empty((2, n), dtype=object), np.zeros((2, n), dtype=bool)
    for c in range(2):
        m = [obj(rng.integers(0, 1 << 62, w, dtype=np.uint64)) for _ in range(2)]
        below, above = m[0] * D + (D - 1) // 2, m[1] * D + (D + 1) // 2
        const = lambda v: np.full(w, v, dtype=object)  # noqa: E731
        far = [c * upto(D >> 60), c * upto(D >> 60), c * upto(D >> 38), c * upto(D >> 38)]
        runs = [below, above, below - (D >> 60) - far[0], above + (D >> 60) + far[1],
                const((D - 1) // 2 - (D >> 38)) - far[2], const((D + 1) // 2 + (D >> 38)) + far[3],
                const(_crt_from_y([0] * len(E), E, D)), const(_crt_from_y([ej - 1 for ej in E], E, D))]
        order = [(k + 3 * c) % 8 for k in range(8)]
        W[c] = np.concatenate([runs[k] for k in order])
        tie[c] = np.concatenate([np.full(w, k < 4) for k in order])
    return W, tie, D


def _check_ties(e, o, l, r, seed=4200, cache=None):
    """ModDown of chosen integers W at level l with r = 0 (relinearize of (0, 0, d)) or r = 1
    (multiply of (0, 1) by (0, d))."""
    cache = {} if cache is None else cache
    t0 = time.time()
    n = _n(e)
    B = 2 if n <= 1 << 12 else 1
    K, A, primes = _kap(e)
    L, lk = e.max_level, l - r
    pids = ks_pids(l, L, K)
    tp = [primes[p] for p in pids]
    what = f"constructed ModDown at N = {n}, K = {K}, A = {A}, level {l}, r = {r}"
    if (l, r) not in cache:
        W, tie, D = _tie_values(tp[lk + 1:], n, seed + 10 * l + r)
        acc = _ntt(o, u64(np.stack([W % p for p in tp], axis=1)), pids, 0)  # (2, l + 1 + K, n)
        ref, amb = moddown_ref(o, acc, l, r, primes, K)
        hi = min(A, l + 1)  # digit 0: its ModUp of the constant 1 is S1 on every limb
        Qd = 1
        for p in primes[:hi]:
            Qd *= p
        S1 = sum(pow(Qd // p, -1, p) * (Qd // p) for p in primes[:hi])
        assert all(S1 % p == 1 for p in primes[:hi]) and all(S1 % p for p in tp)
        key = np.zeros((e.dnum, 2, len(primes), n), dtype=np.uint64)
        for t, p in enumerate(tp):
            key[0, :, pids[t]] = u64((obj(acc[:, t]) * pow(S1 % p, -1, p)) % p)
        d = _pool(primes, l, B, 1, seed + 1, n=n)[:, 0]
        d[:, :hi] = 1  # the constant polynomial 1 in NTT form
        got_acc = ks_acc_ref(o, d[0], l, key, A, primes, K)
        _eq(u64(got_acc), acc, f"{what}: the accumulators of the construction")
        cache[(l, r)] = (W, tie, D, ref, amb, key, d)
    W, tie, D, ref, amb, key, d = cache[(l, r)]
    _eq(amb, tie, f"{what}: the ambiguous coefficients are not exactly the four tie runs")
    assert int(amb.sum()) == 2 * 4 * (n // 8)
    k = _key_from_residues(e, RelinearizationKey, 2, key)
    z = np.zeros((B, 3, l + 1, n), dtype=np.uint64)
    z[:, 2] = d
    if r == 0:
        c = _run(e, o, l, "relinearize", what, lambda: [e.relinearize(e.import_residues(z), k)])[0]
    else:
        one = np.zeros((B, 2, l + 1, n), dtype=np.uint64)
        one[:, 1] = 1

        def fn():
            out = e.multiply(e.import_residues(one), e.import_residues(z[:, 1:]), k)
            out._h
            return [out]
        c = _run(e, o, l, "multiply", what, fn)[0]
    assert (c.level, c.batch, c.npoly, c.is_zero) == (lk, B, 2, False), f"{what}: {c!r}"
    got = e.export_residues(c)
    gc, rc = obj(ntt_poly(o, got, 1)), obj(ntt_poly(o, ref, 1))  # coefficient form
    f = W // D
    X = W % D
    ups = []
    for i in range(lk + 1):
        q = primes[i]
        assert np.array_equal((rc[:, i] - f) % q, np.array(2 * X > D, dtype=object)), "moddown_ref does not round"
        delta = (gc[:, :, i] - f[None]) % q  # (B, 2, n): 0 for floor(W / D), 1 for floor(W / D) + 1
        assert ((delta == 0) | (delta == 1)).all(), \
            f"{what}: limb {i} is neither floor(W / D) nor floor(W / D) + 1 at [batch, poly, coeff] = " \
            f"{np.argwhere((delta != 0) & (delta != 1))[0].tolist()}"
        ups.append(delta == 1)
        for b in range(B):
            bad = (gc[b, :, i] != rc[:, i]) & ~amb
            assert not bad.any(), f"{what}: {int(bad.sum())} coefficients outside the margin differ from the " \
                                  f"integers on limb {i}; first at [poly, coeff] = {np.argwhere(bad)[0].tolist()}"
    ups = np.stack(ups)
    assert (ups == ups[:1]).all(), f"{what}: a coefficient's rounding differs between limbs"
    up = ups[0]  # (B, 2, n)
    _report(what, t0, ambiguous=int(amb.sum()), in_margin_up=int((up[0] & amb).sum()),
            in_margin_down=int((~up[0] & amb).sum()), in_margin_against_nearest=int(((up[0] != (2 * X > D)) & amb).sum()))
    return [got, up]


# ------------------------------------------------------------------------------------------------
# CPU: the oracle alone at N = 2^12, and that the comparison bites
@pytest.fixture(scope="module")
def o12(oracle_lib):
    o = Engine(_lib=oracle_lib, **W12)
    yield o
    _release(o)


def _tiny_ntt(primes, n):
    """A schoolbook negacyclic NTT for the hand case: X_k = sum_i x_i psi^{(2 k + 1) i}."""
    def psi(q):
        return next(pow(a, (q - 1) // (2 * n), q) for a in range(2, q) if pow(a, (q - 1) // 2, q) == q - 1)

    def ntt(limbs, pids, inverse):
        out = []
        for x, p in zip(limbs, pids):
            q = primes[p]
            w = psi(q)
            if inverse:
                out.append([sum(int(x[k]) * pow(w, -(2 * k + 1) * i, q) for k in range(n)) * pow(n, -1, q) % q
                            for i in range(n)])
            else:
                out.append([sum(int(x[i]) * pow(w, (2 * k + 1) * i, q) for i in range(n)) % q for k in range(n)])
        return np.array(out, dtype=np.uint64)
    return ntt


def test_hand_case_n8():
    """n = 8, Q = {17, 97}, P = {113}, one digit (A = 2), d = (5 mod 17, 7 mod 97) constant, key
    b = (2, 3, 4), a = (1, 1, 1) constant.  On paper: (Q_d / q_i)^{-1} = (10, 40), y = (16, 86),
    S = 16 * 97 + 86 * 17 = 3014 = 1365 + Q_d (one overshoot), S mod 113 = 76 (the exact
    conversion would give 1365 mod 113 = 9); acc_b = (10, 21, 304 mod 113 = 78), acc_a = (5, 7, 76);
    ModDown by D = 113: X = 78 > D / 2, conv = -35, out_b = (45 * 14 mod 17, 56 * 91 mod 97) =
    (1, 52); X = 76, conv = -37, out_a = (42 * 14 mod 17, 44 * 91 mod 97) = (10, 27).  Rounding
    down instead (conv = X) gives out_b = (0, 51)."""
    primes, n, K, A, l = [17, 97, 113], 8, 1, 2, 1
    ntt = _tiny_ntt(primes, n)
    one = np.zeros(n, dtype=np.uint64)
    one[0] = 1
    assert ntt([one], [0], 0).tolist() == [[1] * n] and ntt([[1] * n], [2], 1).tolist() == [one.tolist()]
    const = lambda *v: np.array([[x] * n for x in v], dtype=np.uint64)  # noqa: E731
    coef = np.zeros((2, n), dtype=np.uint64)
    coef[:, 0] = 5, 7
    assert modup_ref(coef, primes[:2], primes)[:, 0].tolist() == [5, 7, 76]
    assert modup_ref(coef, primes[:2], primes, exact=True)[:, 0].tolist() == [5, 7, 9]
    key = np.stack([const(2, 3, 4), const(1, 1, 1)])[None]
    acc = ks_acc_ref(ntt, const(5, 7), l, key, A, primes, K)
    assert np.array_equal(u64(acc), np.stack([const(10, 21, 78), const(5, 7, 76)]))
    out, amb = keyswitch_ref(ntt, const(5, 7), l, key, A, primes, K)
    assert np.array_equal(out, np.stack([const(1, 52), const(10, 27)])) and not amb.any()
    out, _ = keyswitch_ref(ntt, const(5, 7), l, key, A, primes, K, floor=True)
    assert np.array_equal(out[0], const(0, 51))
    # r = 1 with the addend (1, 2): D = 97 * 113 = 10961, acc_b + P (1, 2) = (10 + 11, 21 + 2 * 16, 78) =
    # (4, 53, 78); X = 53 mod 97 and 78 mod 113: X = 78 + 113 * 53 = 6067 > D / 2, conv = -4894,
    # 4 + 4894 = 2 mod 17, D = 13 mod 17, 13^{-1} = 4: out_b = 8
    out, amb = keyswitch_ref(ntt, const(5, 7), l, key, A, primes, K, r=1, addend=np.stack([const(1, 2), const(0, 0)]))
    assert out.shape == (2, 1, n) and out[0, 0].tolist() == [8] * n and not amb.any()
    # a non-constant d: the references commute with the ring's product (X^3 d through the same key)
    x = np.zeros((2, n), dtype=np.uint64)
    x[:, 3] = 5, 7
    out3, _ = keyswitch_ref(ntt, ntt(x, [0, 1], 0), l, key, A, primes, K)
    assert ntt(out3[0], [0, 1], 1)[:, 3].tolist() == [1, 52] and int(ntt(out3[0], [0, 1], 1).sum()) == 53
    # the ambiguous mask: 2 X = D - 1 (the constant 56: coefficient 0) is inside any margin, X = 0 is not
    a56 = np.stack([const(0, 0, 56), const(0, 0, 0)])
    _, amb = moddown_ref(ntt, a56, l, 0, primes, K, margin_bits=6)
    assert amb[0, 0] and not amb[0, 1:].any() and not amb[1].any()


def test_references_on_the_oracle(o12):
    """Sections A and B with e = o at N = 2^12 (W12: K = 2, A = 2, L = 4; levels 4, 3 and 1: wide
    digits and a one-limb digit)."""
    o = o12
    assert (o.special_prime_count, o.digit_primes, o.max_level, o.dnum) == (2, 2, 4, 3)
    for l in (4, 3, 1):
        outs = _check_ops(o, o, l, ops=[op for op in OPS if l - RESCALES[op] >= 0])
        assert len(outs) == (6 if l >= 2 else 5)
        for r in (0, 1):
            _check_ties(o, o, l, r)
    _check_ops(o, o, 0, ops=("relinearize", "rotate"))
    _check_key_identity(o, o)


@pytest.mark.parametrize("kw,l,r", [(K16, 16, 0), (K15, 16, 1)], ids=["K16-r0", "K15-r1"])
def test_wide_moddown_on_the_oracle(oracle_lib, kw, l, r):
    """The chains of the unfused ModDown (K + r + 1 = 17 dropped-limb slots) on the oracle."""
    o = Engine(_lib=oracle_lib, **kw)
    try:
        assert o.special_prime_count + r + 1 == 17 and o.max_level >= l
        p = ks_plan(o.special_prime_count, o.digit_primes, l, r, "multiply" if r else "relinearize")
        assert (p["separate"], p["moddown_cols"], p["moddown"]) == (False, 0, 1)
        _check_ops(o, o, l, ops=("multiply",) if r else ("relinearize",))
        _check_ties(o, o, l, r)
    finally:
        _release(o)


def test_the_comparison_bites(o12):
    """Each of these must fail to match the oracle: ModDown rounding down, a ModUp reduced mod
    Q_d, P s' on every limb of the key identity, one flipped residue."""
    o, l = o12, 4
    K, A, primes = _kap(o)
    cache = {}
    got = _check_ops(o, o, l, ops=("relinearize",), cache=cache)[0]
    key, d, out, _ = cache[("relinearize", l, 0)]
    pool = _pool(primes, l, 2, 6, 4100 + l, n=_n(o))
    q = primes[:l + 1]
    assert np.array_equal(_addq(out, pool[:, 3:5], q), got)
    for rule in ("floor", "exact"):
        wrong, _ = keyswitch_ref(o, d, l, key, A, primes, K, **{rule: True})
        assert not np.array_equal(_addq(wrong, pool[:, 3:5], q), got), rule
        differ = (ntt_poly(o, wrong, 1) != ntt_poly(o, out, 1)).all(axis=2)  # per coefficient, on every limb
        if rule == "floor":  # off by one exactly where the nearest integer is above: about half
            assert 0.25 < differ.mean() < 0.75, differ.mean()
        else:  # the overshoot times the key: a polynomial product, seen everywhere
            assert differ.mean() > 0.99, differ.mean()
    bad = got.copy()
    bad[1, 0, 2, 77] ^= 1
    with pytest.raises(AssertionError, match="1 of .* words differ"):
        _eq(bad, _addq(out, pool[:, 3:5], q), "a flipped residue")
    # Section B: rounding down fails on every coefficient above the tie, outside the margin too
    for r in (0, 1):
        c2 = {}
        _check_ties(o, o, l, r, cache=c2)
        W, tie, D, ref, amb, _, _ = c2[(l, r)]
        acc = _ntt(o, u64(np.stack([W % primes[p] for p in ks_pids(l, o.max_level, K)], axis=1)),
                   ks_pids(l, o.max_level, K), 0)
        fl, _ = moddown_ref(o, acc, l, r, primes, K, floor=True)
        d_co = ntt_poly(o, fl, 1) != ntt_poly(o, ref, 1)
        assert np.array_equal(d_co.all(axis=1), np.array(2 * (W % D) > D, dtype=bool)) and (d_co.all(axis=1) & ~amb).any()
        # a narrower margin would not cover the runs D >> 60 from the tie, a wider one takes in D >> 38
        assert int(moddown_ref(o, acc, l, r, primes, K, margin_bits=64)[1].sum()) == 2 * 2 * (_n(o) // 8)
        assert int(moddown_ref(o, acc, l, r, primes, K, margin_bits=36)[1].sum()) == 2 * 6 * (_n(o) // 8)
    # the key identity with P s' on every limb
    for name, kr, s, sp in _key_cases(o, o):
        good = ksk_error_ref(o, kr, s, sp, A, primes, K)
        wrong = ksk_error_ref(o, kr, s, sp, A, primes, K, every_limb=True)
        assert (good == good[:, :1]).all() and not (wrong == wrong[:, :1]).all(), name
        assert max(abs(int(v)) for v in wrong.ravel()) > 1 << 30, name


# ------------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope="module")
def w12(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **W12)
    yield g, o
    _release(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("l", [4, 3, 1])
def test_keyswitch_n12_gpu(w12, l):
    """k_bconv_mfma<., true>: wide digits (levels 4, 3: [2, 2, 1] and [2, 2]) and level 1."""
    g, o = w12
    _both(_check_ops, g, o, l, ops=[op for op in OPS if l - RESCALES[op] >= 0], cache={})
    for r in (0, 1):
        _both(_check_ties, g, o, l, r, cache={})


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_key_identity_n12_gpu(w12):
    _both(_check_key_identity, *w12)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kw,l,r", [(K16, 16, 0), (K15, 16, 1)], ids=["K16-r0", "K15-r1"])
def test_keyswitch_unfused_moddown_gpu(product_lib, oracle_lib, gpu_available, kw, l, r):
    """k_moddown<16>: K + r + 1 = 17 slots."""
    g, o = _pair(product_lib, oracle_lib, **kw)
    try:
        _both(_check_ops, g, o, l, ops=("multiply",) if r else ("relinearize",), cache={})
        _both(_check_ties, g, o, l, r, cache={})
    finally:
        _release(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_keyswitch_n16_gpu(product_lib, oracle_lib, gpu_available):
    """k_bconv_cols<1, true, true> (K = 2): every op at level 3, the products and Section B at 2."""
    g, o = _pair(product_lib, oracle_lib, **W16)
    try:
        _both(_check_ops, g, o, 3, cache={})
        _both(_check_ops, g, o, 2, ops=("relinearize", "multiply"), cache={})
        _both(_check_key_identity, g, o)
        for l in (3, 2):
            for r in (0, 1):
                _both(_check_ties, g, o, l, r, cache={})
    finally:
        _release(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("part", ["relinearize", "multiply", "poly2_int", "l12-rotate", "ties"])
def test_keyswitch_n16_wide_gpu(product_lib, oracle_lib, gpu_available, part):
    """K = 12, A = 12, L = 13 at N = 2^16.  Level 13: relinearize (r = 0, NSTEP 4), multiply
    (r = 1, v in slot 13), poly2_int (r = 2, K + r + 1 = 15); level 12: digits [12, 1], the spread
    path; Section B at level 13 for r = 0 and 1."""
    g, o = _pair(product_lib, oracle_lib, **WIDE16)
    try:
        K, A = 12, 12
        if part == "ties":
            for r in (0, 1):
                _both(_check_ties, g, o, 13, r, cache={})
        elif part == "l12-rotate":
            p = ks_plan(K, A, 12, 0, "rotate")
            assert p["digits"] == [12, 1] and p["spread"] == 1
            _both(_check_ops, g, o, 12, ops=("rotate",), cache={})
        else:
            p = ks_plan(K, A, 13, RESCALES[part], part)
            assert p["moddown_cols"] == 1 and p["moddown_nstep"] == 4 and p["vslot"] == K + RESCALES[part]
            _both(_check_ops, g, o, 13, ops=(part,), cache={})
    finally:
        _release(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_keyswitch_n17_gpu(product_lib, oracle_lib, gpu_available):
    """k_bconv_mfma with rows of 512: one multiply at level 2 and Section B for r = 0."""
    g, o = _pair(product_lib, oracle_lib, **W17)
    try:
        _both(_check_ops, g, o, 2, ops=("multiply",), cache={})
        _both(_check_ties, g, o, 2, 0, cache={})
    finally:
        _release(g, o)

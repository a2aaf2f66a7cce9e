"""Coefficient expansion (include/aesfhe_ext.h aesfhe_expand): Engine.expand,
encrypt_coefficients, create_expansion_keys.

CPU: the oracle has no extension, so the facade runs the steps through aesfhe.h with the monomial
as a coefficient-domain shift; its decrypted int64 coefficients are checked against the coefficient
map within a noise bound computed from the engine's parameters, and the comparison is shown to
bite.  GPU: the HIP engine's aesfhe_expand is residue-exact against that path on the oracle, the
step kernel alone against a coefficient-domain reference made from the GPU's own operands, and
every refused call returns its status and leaves the pool's live bytes where they were."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine

from _int_refs import ntt_poly  # noqa: E402
from _ks_helpers import _drop, _pair, _pool, _profiled  # noqa: E402

ETA = 21  # centred binomial errors: |e| <= 21
SMALL = dict(log_n=10, max_level=6, special_primes=3, seed=31)
LEVEL = 4


# ------------------------------------------------------------------------------------------------
# the noise bound, from the engine's parameters alone
def ks_bound(e, level):
    """Bound on |noise| per coefficient that one key switch at `level` adds: the
    exact ModDown rounds to nearest, eps_0 + eps_1 s with |eps| <= 1/2 and h <= N non-zeros of s,
    plus the key's own errors: digit j's extension has coefficients below alpha_j Q'_j (the fast
    base conversion's sum of alpha_j terms), times an error polynomial |e| <= ETA (N terms per
    coefficient), divided by P."""
    N, A = 1 << e.log_coeff_count, e.digit_primes
    P = math.prod(e.primes[e.max_level + 1:])
    key = 0.0
    for lo in range(0, level + 1, A):
        hi = min(lo + A, level + 1)
        key += N * ETA * (hi - lo) * math.prod(e.primes[lo:hi]) / P
    return (1 + N) / 2 + key


def expand_bound(e, level, n):
    """Steps 0..n-1 of one public-key encryption: step i's key-switch term is doubled by every
    later step (|c +- sigma(c)| <= 2 |c|; the monomial only moves coefficients), sum_i 2^(n-1-i)
    = 2^n - 1 of them; the fresh term v e_pk + e0 + e1 s, |.| <= ETA (1 + N + h), h <= N, comes
    out once, unscaled (the pre-scale cancels the 2^n copies)."""
    N = 1 << e.log_coeff_count
    return ((1 << n) - 1) * ks_bound(e, level) + ETA * (1 + 2 * N)


# ------------------------------------------------------------------------------------------------
# the coefficient map in Python integers (mod Q_level)
def expand_ref(co, first, n, M):
    """(B0, N) integer coefficients -> (B0 2^n, N) after steps first..first+n-1 of DESIGN.md 3.22
    on the plaintext, mod M, centred: pre-scale, X -> X^g in the coefficient domain, sum and
    difference, the negacyclic shift down by 2^j."""
    c = (np.asarray(co).astype(object) * pow(1 << n, -1, M)) % M
    N = c.shape[1]
    for j in range(first, first + n):
        g = (N >> j) + 1
        u = np.zeros_like(c)
        for i in range(N):
            t = (i * g) % (2 * N)
            if t < N:
                u[:, t] = c[:, i]
            else:
                u[:, t - N] = (-c[:, i]) % M
        s, d = (c + u) % M, (c - u) % M
        t = 1 << j
        d = np.roll(d, -t, axis=1)
        d[:, N - t:] = (-d[:, N - t:]) % M
        c = np.concatenate([s, d])
    return np.where(c > M // 2, c - M, c)


def decrypt_coeffs(e, ct, sk):
    co = np.empty((ct.batch, 1 << e.log_coeff_count), dtype=np.int64)
    e._check(e._lib.decrypt(e._h, sk._h, ct._h, co.ctypes.data_as(C.POINTER(C.c_int64))))
    return co


def max_dev(got, want):
    return int(np.abs(got.astype(object) - want).max())


@pytest.fixture(scope="module")
def small(oracle_lib):
    e = Engine(_lib=oracle_lib, **SMALL)
    sk = e.create_secret_key(1)
    return e, sk, e.create_public_key(sk), e.create_expansion_keys(sk, 0, 10)


_FULL = {}


def _full(small, n):
    """One full expansion of n steps, shared by the tests that read it: (input coefficients,
    decrypted output coefficients)."""
    if n not in _FULL:
        e, sk, pk, xk = small
        N = 1 << e.log_coeff_count
        rng = np.random.default_rng(n)
        delta = int(round(e.scales[LEVEL]))
        co = np.zeros((1, N), dtype=np.int64)
        co[0, :1 << n] = delta * (1 - 2 * rng.integers(0, 2, 1 << n))
        ct = e.encrypt_coefficients(co, pk, LEVEL)
        out = e.expand(ct, xk[:n])
        assert (out.batch, out.level, out.npoly) == (1 << n, LEVEL, 2)
        _FULL[n] = (co, decrypt_coeffs(e, out, sk))
    return _FULL[n]


# ------------------------------------------------------------------------------------------------
# CPU, on the oracle
@pytest.mark.parametrize("n", [5, 10])
def test_full_expansion_gives_one_constant_polynomial_per_coefficient(small, n):
    _check_full(small[0], *_full(small, n), n)


def _check_full(e, co, dec, n):
    bound = expand_bound(e, LEVEL, n)
    assert bound < e.scales[LEVEL] / 2 ** 10, "the bound must separate +-Delta from noise"
    want = np.zeros(dec.shape, dtype=object)
    want[:, 0] = co[0, :1 << n]  # output t is the constant polynomial a_t
    M = math.prod(e.primes[:LEVEL + 1])
    assert np.array_equal(expand_ref(co, 0, n, M), want), "the integer reference is not the coefficient map"
    worst = max_dev(dec, want)
    print(f"n={n}: max |decrypted - expected| = {worst} (bound {bound:.0f}, Delta/2^10 = {e.scales[LEVEL] / 1024:.3g})")
    assert worst <= bound


def test_nonzero_first_step_and_batched_input(small):
    """Steps 3 and 4 on B0 = 3 dense random elements: element t B0 + b of the result holds input
    b's coefficient 8 (t + 4 w) at index 32 w, and zero at the other multiples of 8.  (The input's
    coefficients at indices that are no multiple of 2^first are outside the map: earlier steps
    would have cleared them; they stay at such indices and are not read here.)"""
    e, sk, pk, xk = small
    N, first, n, B0 = 1 << e.log_coeff_count, 3, 2, 3
    rng = np.random.default_rng(7)
    co = rng.integers(-2 ** 30, 2 ** 30, (B0, N), dtype=np.int64)
    out = e.expand(e.encrypt_coefficients(co, pk, LEVEL), xk[first:first + n], first=first)
    assert (out.batch, out.level) == (B0 << n, LEVEL)
    dec = decrypt_coeffs(e, out, sk)
    want = np.zeros((B0 << n, N // 8), dtype=object)
    for t in range(1 << n):
        for b in range(B0):
            want[t * B0 + b, ::4] = co[b, 8 * t::32]
    # two steps: the first key-switch term doubled once; the fresh term once
    bound = 3 * ks_bound(e, LEVEL) + ETA * (1 + 2 * N)
    assert bound < 2 ** 30 / 2 ** 10
    worst = max_dev(dec[:, ::8], want)
    print(f"first=3, n=2, B0=3: max |decrypted - expected| = {worst} (bound {bound:.0f})")
    assert worst <= bound
    # the same map from the integer reference on the multiples of 8 alone
    sparse = np.zeros_like(co)
    sparse[:, ::8] = co[:, ::8]
    ref = expand_ref(sparse, first, n, math.prod(e.primes[:LEVEL + 1]))
    assert np.array_equal(ref[:, ::8], want) and not ref[:, 1::8].any()


def _no_negation(self, ct, t):
    """Engine._monomial_shift without the negation of the wrapped tail (a cyclic shift)."""
    from aes_xor_fhe.fhe import _as_ptr
    res = self.export_residues(ct)
    flat = np.ascontiguousarray(res.reshape(-1, res.shape[-1]))
    pids = np.ascontiguousarray(np.arange(flat.shape[0], dtype=np.int32) % res.shape[2])
    for inv in (1, 0):
        self._check(self._lib.ntt_host(self._h, _as_ptr(flat, C.c_uint64), flat.shape[0], _as_ptr(pids, C.c_int32), inv))
        if inv:
            flat = np.ascontiguousarray(np.roll(flat, -t, axis=1))
    return self.import_residues(flat.reshape(res.shape))


@pytest.mark.parametrize("mutation", ["plus-and-minus-swapped", "wrapped-tail-not-negated", "shift-2^j+1"])
def test_the_comparison_bites(small, monkeypatch, mutation):
    """A wrong checker does not pass the full expansion's assertion: the oracle path with the sum
    and the difference swapped, with a cyclic instead of a negacyclic shift, with the shift 2^j + 1."""
    e, sk, pk, xk = small
    co, _ = _full(small, 5)
    if mutation == "plus-and-minus-swapped":
        add, sub = e._lib.add, e._lib.sub
        monkeypatch.setattr(e._lib, "add", sub)
        monkeypatch.setattr(e._lib, "sub", add)
    elif mutation == "wrapped-tail-not-negated":
        monkeypatch.setattr(Engine, "_monomial_shift", _no_negation)
    else:
        right = Engine._monomial_shift
        monkeypatch.setattr(Engine, "_monomial_shift", lambda self, ct, t: right(self, ct, t + 1))
    dec = decrypt_coeffs(e, e.expand(e.encrypt_coefficients(co, pk, LEVEL), xk[:5]), sk)
    monkeypatch.undo()
    with pytest.raises(AssertionError):
        _check_full(e, co, dec, 5)


def test_zero_input_and_refused_calls_oracle(small):
    e, sk, pk, xk = small
    z = e.expand(e.zeros(3, LEVEL), xk[:2])
    assert z.is_zero and (z.batch, z.level) == (12, LEVEL) and not e.export_residues(z).any()
    ct = e.encrypt_coefficients(np.ones(1 << e.log_coeff_count, dtype=np.int64), pk, LEVEL)
    with pytest.raises(RuntimeError, match="galois element"):
        e.expand(ct, xk[1:3])
    with pytest.raises(RuntimeError, match="not within"):
        e.expand(ct, xk[8:], first=9)
    with pytest.raises(RuntimeError, match="not within"):
        e.expand(ct, [])
    with pytest.raises(RuntimeError, match="not a galois key"):
        e.expand(ct, [e.create_relinearization_key(sk)])
    with pytest.raises(RuntimeError, match="2 polynomials"):
        e.expand(e._call_ct(e._lib.tensor, ct._h, ct._h), xk[:1])
    with pytest.raises(ValueError):
        e.encrypt_coefficients(np.ones((1, 8), dtype=np.int64), pk, LEVEL)
    with pytest.raises(ValueError):
        e.create_expansion_keys(sk, 8, 3)


def test_product_never_takes_the_oracle_path(small, monkeypatch):
    e, sk, pk, xk = small
    ct = e.encrypt_coefficients(np.ones(1 << e.log_coeff_count, dtype=np.int64), pk, LEVEL)
    monkeypatch.setattr(Engine, "on_device", property(lambda self: True))
    with pytest.raises(RuntimeError, match="rebuild it"):
        e.expand(ct, xk[:1])


# ------------------------------------------------------------------------------------------------
# GPU: residues
W12 = dict(log_n=12, max_level=4, special_primes=3, scale_bits=42, seed=21)  # both prime classes (test_integer_witnesses)
W16 = dict(log_n=16, max_level=4, special_primes=3, seed=23)
W16D = dict(log_n=16, max_level=12, special_primes=10, digit_primes=12, scale_bits=40, seed=25)
W17 = dict(log_n=17, max_level=2, special_primes=2, seed=24)
_ENG = {}


def _engines(product_lib, oracle_lib, name, kw, first, n):
    """(HIP engine, oracle, their expansion keys for steps first..first+n-1), one pair per chain;
    keys made on demand and kept."""
    if name not in _ENG:
        for k in [k for k in _ENG if k != name]:
            g, o = _ENG.pop(k)[:2]
            _drop(g, o)
        g, o = _pair(product_lib, oracle_lib, **kw)
        _ENG[name] = (g, o, g.create_secret_key(9), o.create_secret_key(9), {}, {})
    g, o, skg, sko, kg, ko = _ENG[name]
    for j in range(first, first + n):
        if j not in kg:
            kg[j], ko[j] = g.create_expansion_keys(skg, j, 1)[0], o.create_expansion_keys(sko, j, 1)[0]
    return g, o, [kg[j] for j in range(first, first + n)], [ko[j] for j in range(first, first + n)]


def _parity(product_lib, oracle_lib, name, kw, first, n, B0, level=None):
    g, o, kg, ko = _engines(product_lib, oracle_lib, name, kw, first, n)
    level = g.max_level if level is None else level
    arr = _pool(g.primes, level, B0, 2, 100 * first + n, n=1 << g.log_coeff_count)
    out, prof = _profiled(g, lambda: g.expand(g.import_residues(arr), kg, first=first))
    assert prof.get("expand_step", 0) == n and prof.get("expand_scale", 0) == 1 and prof.get("expand_mono", 0) == 1, prof
    want = o.expand(o.import_residues(arr), ko, first=first)
    assert (out.batch, out.level, out.npoly) == (want.batch, want.level, want.npoly) == (B0 << n, level, 2)
    a, b = g.export_residues(out), o.export_residues(want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{name} steps ({first}, {n}), B0 {B0}: {len(bad)} of {a.size} residues differ; first at "
                             f"[batch, poly, limb, coeff] = {bad[0].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("first,n,B0", [(0, 3, 1), (9, 3, 3)])
def test_expand_residue_exact_generic_ntt(product_lib, oracle_lib, gpu_available, first, n, B0):
    """N = 2^12, the 50-bit q_0 and limbs on both sides of 2^42; (9, 3): the last steps, g down to
    3, shift N/2, a batch that is no power of two."""
    _parity(product_lib, oracle_lib, "w12", W12, first, n, B0)


@pytest.mark.gpu
@pytest.mark.parametrize("first,n", [(0, 2), (4, 3)])
def test_expand_residue_exact_fused_ntt(product_lib, oracle_lib, gpu_available, first, n):
    _parity(product_lib, oracle_lib, "w16", W16, first, n, 2)


@pytest.mark.gpu
def test_expand_residue_exact_wide_digits(product_lib, oracle_lib, gpu_available):
    """special_primes = 10, digit_primes = 12 at L = 12: the fused key switch with a 12-prime digit."""
    _parity(product_lib, oracle_lib, "w16d", W16D, 0, 2, 2)


@pytest.mark.gpu
def test_expand_residue_exact_n17(product_lib, oracle_lib, gpu_available):
    _parity(product_lib, oracle_lib, "w17", W17, 0, 2, 1)


@pytest.mark.gpu
def test_expand_of_zero_is_zero(product_lib, oracle_lib, gpu_available):
    g, o, kg, ko = _engines(product_lib, oracle_lib, "w12", W12, 0, 3)
    z = g.expand(g.zeros(3, 2), kg)
    assert z.is_zero and (z.batch, z.level, z.npoly) == (24, 2, 2) and not g.export_residues(z).any()


def _step_ref(g, o, arr, key, first):
    """One step from the HIP engine's own operands: c' = arr / 2 in Python integers, u = the
    engine's aesfhe_galois of c'; then c' + u and (c' - u) shifted down by 2^first in the
    coefficient domain (the oracle's ntt_host; no multiplication by a root)."""
    B, _, nl, N = arr.shape
    q = np.array(g.primes[:nl], dtype=object)[None, None, :, None]
    c = (arr.astype(object) * np.array([pow(2, -1, p) for p in g.primes[:nl]], dtype=object)[None, None, :, None]) % q
    cg = g.import_residues(c.astype(np.uint64))
    u = g.export_residues(g._call_ct(g._lib.galois, cg._h, key._h)).astype(object)
    s, d = (c + u) % q, (c - u) % q
    co = ntt_poly(o, d.astype(np.uint64), 1).astype(object)
    t = 1 << first
    co = np.roll(co, -t, axis=-1)
    co[..., N - t:] = (-co[..., N - t:]) % q
    return np.concatenate([s.astype(np.uint64), ntt_poly(o, co.astype(np.uint64), 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("w12", W12), ("w16", W16)])
def test_step_kernel_alone(product_lib, oracle_lib, gpu_available, name, kw):
    """(first, 1) for first = 0, 7 and logN - 1 against the reference made from the GPU's own c and
    galois output: the new kernels isolated from the key switch."""
    for first in (0, 7, kw["log_n"] - 1):
        g, o, kg, _ = _engines(product_lib, oracle_lib, name, kw, first, 1)
        arr = _pool(g.primes, 2, 2, 2, 50 + first, n=1 << g.log_coeff_count)
        got = g.export_residues(g.expand(g.import_residues(arr), kg, first=first))
        want = _step_ref(g, o, arr, kg[0], first)
        assert np.array_equal(got, want), f"{name} step {first}: {np.argwhere(got != want)[:1].tolist()}"


@pytest.mark.gpu
def test_refused_calls_return_their_status_and_take_nothing(product_lib, oracle_lib, gpu_available):
    chain = dict(log_n=12, max_level=4, special_primes=2, digit_primes=2, seed=23)  # 3 digits at the top (test_error_paths)
    e = Engine(_lib=product_lib, **chain)
    sk = e.create_secret_key(2)
    xk = e.create_expansion_keys(sk, 0, 3)
    trimmed = e.create_expansion_keys(sk, 0, 1)[0]
    e.trim_key(trimmed, 1)
    ct = e.import_residues(_pool(e.primes, 4, 2, 2, 3, n=1 << 12))
    three = e._call_ct(e._lib.tensor, ct._h, ct._h)
    rlk, hk = e.create_relinearization_key(sk), e.create_hoisted_rotation_key(sk, 1)
    last = e.create_expansion_keys(sk, 11, 1)
    ok = e.expand(ct, xk)  # anything made on first use exists before the baseline
    del ok
    gc.collect()
    e.synchronize()
    base = e.pool_stats()["live"]

    def status(c, keys, first=0):
        arr = (C.c_void_p * len(keys))(*[k._h for k in keys])
        out = C.c_void_p()
        rc = e._lib.expand(e._h, c._h, first, len(keys), arr, C.byref(out))
        assert not out.value
        return rc, e._lib.last_error().decode()

    EARG, EDEGREE, ELEVEL = -1, -4, -5
    for what, args, code, text in [
            ("wrong galois element", (ct, [xk[1]]), EARG, "galois element"),
            ("a hoisted key", (ct, [hk]), EARG, "not a galois key"),
            ("a relinearisation key", (ct, [rlk]), EARG, "not a galois key"),
            ("first + n > logN", (ct, last + last, 11), EARG, "not within"),
            ("three polynomials", (three, xk[:1]), EDEGREE, "2 polynomials"),
            ("a key trimmed below the level", (ct, [trimmed]), ELEVEL, "trimmed")]:
        rc, msg = status(*args)
        assert rc == code and text in msg, (what, rc, msg)
        e.synchronize()
        assert e.pool_stats()["live"] == base, what
    with pytest.raises(RuntimeError, match="trimmed"):
        e.expand(ct, [trimmed])
    # and a permitted call afterwards still runs
    assert e.expand(ct, xk).batch == 16

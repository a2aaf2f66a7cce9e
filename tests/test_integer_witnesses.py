"""Client-path and bootstrap primitives against references in Python integers.

The GPU suites compare the HIP engine with the CPU oracle residue for residue; where the oracle is
itself pinned (the NTT's schoolbook KAT, FIPS-197, the golden traces) that is a strong check, but
for most primitives an error of rounding or of an integer edge that both implementations share
would pass.  Here each of the following has a third witness, a few lines of Python integers in
_int_refs.py, whose only compiled ingredient is the oracle's ntt_host:

  1  signed coefficients -> residues (k_coeffs_res: encrypt, encrypt_device, pt_create, and
     pt_create_ext's P limbs through one key-less linear_bsgs, oracle only)
  2  decrypt: c0 + c1 s + c2 s^2, the 128-bit CRT of limbs 0 and 1, centring at Q / 2, saturation
  3  ModRaise (k_lift0)
  4  mul_i
  5  the automorphism with c1 = 0 (k_galois and the fused paths' permuted reads)
  6  rescale and the level-down constant folded into it
  7  dot_pt (k_dot_pt)
  8  the device codec's rounding ties and overflow guard (k_sfft_round)

Every comparison is np.array_equal.  Each `_check_*` function runs one section on an engine `e`
with the references' NTTs on the oracle `o`; the CPU tests call it with e = o at N = 2^12 (so a
reference cannot drift unnoticed without a GPU) and show that the comparison bites (the wrong
centring rule, no saturation, round-half-even, a perturbed result must fail); the GPU tests call
it on the HIP engine and on the oracle and compare the two results as well."""
import ctypes as C

import numpy as np
import pytest
import torch

from aes_xor_fhe._abi import c_ct_p, c_key_p, c_pt_p
from aes_xor_fhe.fhe import Engine, FixedRotationKey, _Owned

from _int_refs import (I64_MAX, centre, crt2, decrypt_ref, dot_pt_sum_ref, galois_ref, level_down_const_ref,  # noqa: E402
                       lift_ref, mul_i_ref, ntt_limbs, ntt_poly, obj, rescale_ref, residues_ref, round_tie, u64)
from _ks_helpers import _drop, _pair, _pool  # noqa: E402
from test_range_bounds import (_centre_ct, _check_centre, _classes, _const_pool, _edge_pool,  # noqa: E402
                               _level_down_const)

W12 = dict(log_n=12, max_level=4, special_primes=2, scale_bits=42, seed=21)
W12_CLASSES = "BsBBs"  # q_0..q_4 against 2^42 (kernels.h kBigPrime), written from an oracle run and pinned below
W12D = dict(W12, scale_bits=None)  # the default scale
W16 = dict(log_n=16, max_level=3, special_primes=2, seed=23)
W17 = dict(log_n=17, max_level=2, special_primes=2, seed=24)
# decrypt: Q = q0 q1 near 2^92 / 2^94 (saturation reachable), q1 > q0, Q < 2^63
DEC_CHAINS = {"w12": W12, "w12-default-scale": W12D, "q1>q0": dict(W12, base_bits=36, scale_bits=44),
              "Q<2^63": dict(W12, base_bits=30, scale_bits=30)}
I64_MIN = -(1 << 63)
ROTS2, ROTS3 = [[0, 3], [5, 6]], [[0, 3, 7], [5, 6, 2]]


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _n(e):
    return 1 << e.log_coeff_count


def _runs(values, n, rng, draw, rot=0):
    """n words in equal runs, one per entry of `values`, the rest of the runs drawn by draw(rng,
    count); the runs rotated by `rot` places."""
    nrun = 1
    while nrun < len(values) + max(2, len(values) // 4):
        nrun *= 2
    w = n // nrun
    assert w >= 1
    runs = [np.full(w, v, dtype=object) for v in values]
    runs += [draw(rng, w) for _ in range(nrun - len(values))]
    runs = runs[rot % nrun:] + runs[:rot % nrun]
    return np.concatenate(runs)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ; first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def _both(check, g, o, *args, **kw):
    """One section on the HIP engine and on the oracle, each against the integers; then the two
    results against each other."""
    rg, ro = check(g, o, *args, **kw), check(o, o, *args, **kw)
    assert len(rg) == len(ro)
    for i, (a, b) in enumerate(zip(rg, ro)):
        _eq(a, b, f"{check.__name__}: HIP engine vs oracle, result {i}")
    return rg


@pytest.fixture(scope="module")
def o12(oracle_lib):
    return Engine(_lib=oracle_lib, **W12)


@pytest.fixture(scope="module")
def w12(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **W12)
    yield g, o
    _drop(g, o)


@pytest.fixture(scope="module")
def w16(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **W16)
    yield g, o
    _drop(g, o)


def test_witness_chains_on_the_oracle(o12, oracle_lib):
    """W12 has both prime classes among its levels and at the two levels the rescale tests use."""
    l = o12.max_level
    assert _classes(o12.primes[:l + 1]) == W12_CLASSES and W12_CLASSES[l] != W12_CLASSES[l - 1]
    assert all(q < o12.primes[0] >> 1 for q in o12.primes[1:l + 1])


# ------------------------------------------------------------------------------------------------
# 1. coefficients -> residues
def _coeff_rows(primes, n, B, seed):
    """(B, n) int64 in equal runs of 0, 1, -1, INT64_MAX, INT64_MIN, INT64_MIN + 1, +-2^62, for
    every prime (special primes included) +-q, +-(q - 1), +-5 q, and seeded random int64."""
    vals = [0, 1, -1, I64_MAX, I64_MIN, I64_MIN + 1, 1 << 62, -(1 << 62)]
    for q in primes:
        vals += [q, -q, q - 1, -(q - 1), 5 * q, -5 * q]
    assert all(I64_MIN <= v <= I64_MAX for v in vals)
    rng = np.random.default_rng(seed)
    draw = lambda r, w: r.integers(I64_MIN, I64_MAX, w, dtype=np.int64, endpoint=True).astype(object)  # noqa: E731
    rows = np.stack([_runs(vals, n, rng, draw, rot=3 * b) for b in range(B)])
    return np.array(rows, dtype=np.int64), vals


def _encrypt_raw(e, key, co, level, nonce, device):
    co = np.ascontiguousarray(co, dtype=np.int64)
    out = C.c_void_p()
    if device:
        t = torch.from_numpy(co).to(e.client_device)
        e._torch_sync()
        e._check(e._lib.encrypt_device(e._h, key._h, t.data_ptr(), co.shape[0], level, nonce, C.byref(out)))
        e.synchronize()
    else:
        e._check(e._lib.encrypt(e._h, key._h, _p64(co), co.shape[0], level, nonce, C.byref(out)))
    return e._ct(out.value)


def _pt_create(e, co, level, ext=False):
    co = np.ascontiguousarray(co, dtype=np.int64)
    out = C.c_void_p()
    e._check((e._lib.pt_create_ext if ext else e._lib.pt_create)(e._h, _p64(co), level, C.byref(out)))
    h = _Owned(e._lib, out.value, e._lib.pt_free)
    h.engine = e
    return h


def _pt_residues(e, pt, level):
    """The residues of a pt_create handle made at `level`: add_pt to an imported all-zero
    ciphertext, polynomial 0 (polynomial 1 stays zero)."""
    z = e.import_residues(np.zeros((1, 2, level + 1, _n(e)), dtype=np.uint64))
    a = e.export_residues(e._call_ct(e._lib.add_pt, z._h, pt._h))
    assert not a[:, 1].any(), "add_pt touched polynomial 1"
    return a[0, 0]


def _check_coeffs_res(e, o, seed=101):
    """c0(x) - c0(0) under one key and nonce is NTT(x mod q) and c1 does not change: public and
    secret key, host and device coefficients, batch 2, top level; pt_create at the top level and
    one below."""
    l, n = e.max_level, _n(e)
    primes = e.primes[:l + 1]
    rows, _ = _coeff_rows(e.primes, n, 2, seed)
    want = ntt_poly(o, residues_ref(rows, primes), 0)  # (2, l + 1, n)
    sk = e.create_secret_key(9)
    pk = e.create_public_key(sk)
    outs = []
    for kn, key in (("public", pk), ("secret", sk)):
        for device in (False, True):
            nonce = 7000 + 2 * (kn == "secret") + device
            cx = e.export_residues(_encrypt_raw(e, key, rows, l, nonce, device))
            cz = e.export_residues(_encrypt_raw(e, key, np.zeros_like(rows), l, nonce, device))
            what = f"encrypt{'_device' if device else ''} under the {kn} key"
            _eq(cx[:, 1], cz[:, 1], f"{what}: c1 depends on the message")
            diff = np.stack([(cx[:, 0, i] + np.uint64(q) - cz[:, 0, i]) % np.uint64(q) for i, q in enumerate(primes)],
                            axis=1)
            _eq(diff, want, f"{what}: c0(x) - c0(0) vs NTT(x mod q)")
            outs.append(cx)
    for lv in (l, l - 1):
        for b in range(2):
            got = _pt_residues(e, _pt_create(e, rows[b], lv), lv)
            _eq(got, want[b, :lv + 1], f"pt_create at level {lv}, row {b}")
            outs.append(got)
    return outs


def _bsgs_identity(e, ct, pt):
    """aesfhe_linear_bsgs with one key-less giant and one identity baby: ct * pt over Q_l u P, one
    ModDown with the rescale."""
    bk, gk = (c_key_p * 1)(None), (c_key_p * 1)(None)
    nterm, tb, pts = (C.c_int32 * 1)(1), (C.c_int32 * 1)(0), (c_pt_p * 1)(pt._h)
    return e._call_ct(e._lib.linear_bsgs, ct._h, 1, bk, 1, gk, nterm, tb, pts)


def _pt_ext_products(e, seed=101):
    """pt_create_ext of the edge rows, consumed by the key-less linear_bsgs (the only reader of
    its P limbs in the ABI)."""
    l, n = e.max_level, _n(e)
    rows, _ = _coeff_rows(e.primes, n, 2, seed)
    ct = e.import_residues(_edge_pool(e.primes, l, ROTS2, 55, n=n))
    outs = []
    for b in range(2):
        r = _bsgs_identity(e, ct, _pt_create(e, rows[b], l, ext=True))
        assert (r.level, r.batch, r.npoly) == (l - 1, 2, 2)
        outs.append(e.export_residues(r))
    return outs


def test_coeff_residues_on_the_oracle(o12):
    rows, vals = _coeff_rows(o12.primes, _n(o12), 2, 101)
    for b in range(2):
        assert set(vals) <= set(rows[b].tolist())
        assert len(set(rows[b].tolist())) > len(vals) + _n(o12) // 8  # the random runs
    outs = _check_coeffs_res(o12, o12)
    # the comparison bites: one residue off by one, and the k_coeffs_res rule without its "+ 1"
    primes = o12.primes[:o12.max_level + 1]
    want = residues_ref(rows, primes)
    assert int(want[0, 0][rows[0] == I64_MIN][0]) == (I64_MIN % primes[0])
    wrong = np.stack([np.where(rows >= 0, obj(rows) % q, q - ((-obj(rows)) % q)) for q in primes], axis=1)
    assert (obj(want) != wrong).any()  # differs exactly at the negative multiples of q (q, not 0)
    bad = want.copy()
    bad[1, 2, 17] ^= 1
    assert not np.array_equal(ntt_poly(o12, bad, 0)[1, 2], outs[-3][2]) and \
        np.array_equal(ntt_poly(o12, want, 0)[1, 2], outs[-3][2])
    assert len(_pt_ext_products(o12)) == 2  # the plan is accepted


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_coeff_residues_gpu(w12):
    """Section 1 at N = 2^12.  pt_create_ext is compared with the oracle only (its P limbs are not
    readable through the ABI): the key-less linear_bsgs product of the same rows on both engines."""
    g, o = w12
    _both(_check_coeffs_res, g, o)
    for i, (a, b) in enumerate(zip(_pt_ext_products(g), _pt_ext_products(o))):
        _eq(a, b, f"linear_bsgs with a pt_create_ext plaintext, row {i}: HIP engine vs oracle")


# ------------------------------------------------------------------------------------------------
# 2. decrypt
def _dec_values(q0, q1, n, seed, rot=0):
    """n Python integers: runs of the edges of the CRT, the centring and the saturation, of random
    values below 2^62 in magnitude and of random values over all of [0, Q).  q1 None: level 0."""
    rng = np.random.default_rng(seed)
    big = lambda r, w, hi: np.array([int.from_bytes(r.bytes(16), "little") % hi for _ in range(w)], dtype=object)  # noqa: E731
    if q1 is None:
        vals = [0, 1, -1, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
        return _runs(vals, n, rng, lambda r, w: big(r, w, q0), rot)
    Q = q0 * q1
    vals = [0, 1, -1]
    for m in ((1 << 63) - 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1):
        vals += [m, -m]
    vals += [Q // 2, Q // 2 + 1, Q - 1, q0, q1, q0 * (q1 - 1), 3 * q1]
    state = {"k": 0}

    def draw(r, w):  # alternately small (signed, below 2^62) and over all of [0, Q)
        state["k"] += 1
        if state["k"] % 2:
            return big(r, w, 1 << 63) - (1 << 62)
        return big(r, w, Q)
    return _runs(vals, n, rng, draw, rot)


def _import_ints(e, o, x, level, garbage=None):
    """The (B, 2, level + 1, n) ciphertext with c1 = 0 and c0 limb i = NTT_i(x mod q_i); garbage
    (a seed): limbs 2.. hold random residues instead, which decrypt must not read."""
    B, n = x.shape
    arr = np.zeros((B, 2, level + 1, n), dtype=np.uint64)
    arr[:, 0] = ntt_poly(o, residues_ref(x, e.primes[:level + 1]), 0)
    if garbage is not None and level >= 2:
        arr[:, :, 2:] = _pool(e.primes, level, B, 2, garbage, n=n)[:, :, 2:]
    return arr


def _decrypt_raw(e, sk, ct, device):
    n = _n(e)
    if device:
        t = torch.empty((ct.batch, n), dtype=torch.int64, device=e.client_device)
        e._torch_sync()
        e._check(e._lib.decrypt_device(e._h, sk._h, ct._h, t.data_ptr()))
        e.synchronize()
        return t.cpu().numpy()
    co = np.empty((ct.batch, n), dtype=np.int64)
    e._check(e._lib.decrypt(e._h, sk._h, ct._h, _p64(co)))
    return co


def _dec_inputs(e, level):
    q0, q1 = e.primes[0], (e.primes[1] if level >= 1 else None)
    x = np.stack([_dec_values(q0, q1, _n(e), 300 + b, rot=5 * b) for b in range(2)])
    return x, q0 * (q1 or 1)


def _check_decrypt_values(e, o, level):
    """decrypt and decrypt_device of chosen integers are sat(centre(x mod Q))."""
    x, Q = _dec_inputs(e, level)
    want = decrypt_ref(x, Q)
    sk = e.create_secret_key(9)
    ct = e.import_residues(_import_ints(e, o, x, level, garbage=17))
    outs = []
    for device in (False, True):
        got = _decrypt_raw(e, sk, ct, device)
        _eq(got, want, f"decrypt{'_device' if device else ''} at level {level}")
        outs.append(got)
    return outs


def _secret_residues(e, sk):
    """aesfhe_key_export of a secret key: (primes, N) NTT-domain residues."""
    kind, g, seed, words = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_int64()
    e._check(e._lib.key_export(e._h, sk._h, C.byref(kind), C.byref(g), C.byref(seed), C.byref(words), None))
    data = np.empty(words.value, dtype=np.uint64)
    e._check(e._lib.key_export(e._h, sk._h, C.byref(kind), C.byref(g), C.byref(seed), C.byref(words),
                               data.ctypes.data_as(C.POINTER(C.c_uint64))))
    assert kind.value == 0 and words.value == len(e.primes) * _n(e)
    return data.reshape(len(e.primes), _n(e))


def _check_decrypt_secret(e, o, level, B):
    """decrypt of 2- and 3-polynomial ciphertexts of chosen residues: c0 + c1 s (+ c2 s^2) mod q
    pointwise in Python integers, limbs 0 and 1, the oracle's inverse NTT, CRT, centre, saturate."""
    n = _n(e)
    sk = e.create_secret_key(9)
    s = obj(_secret_residues(e, sk))
    q0, q1 = e.primes[0], e.primes[1]
    outs = []
    for npoly, rots in ((2, ROTS2), (3, ROTS3)):
        arr = _edge_pool(e.primes, level, rots[:B], 400 + npoly, n=n)
        m = []
        for i, q in ((0, q0), (1, q1)):
            c = obj(arr[:, :, i])
            v = c[:, 0] + c[:, 1] * s[i] + (c[:, 2] * s[i] * s[i] if npoly == 3 else 0)
            m.append(ntt_limbs(o, u64(v % q), [i] * B, 1))
        want = decrypt_ref(crt2(m[0], m[1], q0, q1), q0 * q1)
        ct = e.import_residues(arr)
        for device in (False, True):
            got = _decrypt_raw(e, sk, ct, device)
            _eq(got, want, f"decrypt{'_device' if device else ''} of {npoly} polynomials at level {level}")
            outs.append(got)
    return outs + [u64(s)]


@pytest.mark.parametrize("chain", list(DEC_CHAINS))
def test_decrypt_on_the_oracle(oracle_lib, chain):
    kw = {k: v for k, v in DEC_CHAINS[chain].items() if v is not None}
    o = Engine(_lib=oracle_lib, **kw)
    q0, q1 = o.primes[:2]
    Q = q0 * q1
    assert (chain == "Q<2^63") == (Q < 1 << 63) and (q1 > q0 if chain == "q1>q0" else q1 < q0 or Q < 1 << 63)
    x, _ = _dec_inputs(o, 1)
    # the stated input condition: at most half of the words saturate, at least an eighth are
    # unsaturated random values (random: not one of the edge runs, i.e. seen once)
    c = centre(x % Q, Q)
    sat = np.array(abs(c) > I64_MAX, dtype=bool)
    vals, counts = np.unique(np.array([int(v) % Q for v in x.ravel()], dtype=object), return_counts=True)
    once = set(vals[counts == 1].tolist())
    rnd = np.array([int(v) % Q in once for v in x.ravel()]).reshape(x.shape)
    assert sat.mean() <= 0.5 and (rnd & ~sat).mean() >= 0.125, (sat.mean(), (rnd & ~sat).mean())
    assert (sat.mean() == 0) == (chain == "Q<2^63")
    for v in (Q // 2, Q // 2 + 1, q0 * (q1 - 1), 3 * q1, (1 << 63) - 1, -(1 << 63)):
        assert (x[0] == v).any()
    host, _ = _check_decrypt_values(o, o, 1)
    # the comparison bites: centring with >= and a conversion without the clamp both differ
    assert not np.array_equal(decrypt_ref(x, Q, ge=True), host)
    if chain != "Q<2^63":
        assert not np.array_equal(decrypt_ref(x, Q, sat=False), host)
    if chain == "w12":
        x0, _ = _dec_inputs(o, 0)
        for v in ((q0 - 1) // 2, (q0 + 1) // 2, q0 - 1):
            assert (x0[0] == v).any()
        h0, _ = _check_decrypt_values(o, o, 0)
        assert not np.array_equal(decrypt_ref(x0, q0, ge=True), h0)
        _check_decrypt_values(o, o, 3)
        outs = _check_decrypt_secret(o, o, 1, 2)
        bad = outs[0].copy()
        bad[1, 5] += 1
        assert not np.array_equal(bad, outs[1])


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("chain", list(DEC_CHAINS))
def test_decrypt_gpu(product_lib, oracle_lib, gpu_available, chain):
    kw = {k: v for k, v in DEC_CHAINS[chain].items() if v is not None}
    g, o = _pair(product_lib, oracle_lib, **kw)
    try:
        _both(_check_decrypt_values, g, o, 1)
        if chain == "w12":
            _both(_check_decrypt_values, g, o, 0)
            _both(_check_decrypt_values, g, o, 3)
            _both(_check_decrypt_secret, g, o, 1, 2)
    finally:
        _drop(g, o)


# ------------------------------------------------------------------------------------------------
# 3. ModRaise
def _lift_pattern(primes, L, n, rng, rot):
    """Limb 0 in coefficient form: 0, 1, (q0 - 1) / 2, (q0 + 1) / 2, q0 - 1, per target limb
    q0 - q_i and q0 - 3 q_i (negative with remainder zero: the m == 0 branch) and q_i mod q0, and
    random values."""
    q0 = primes[0]
    vals = [0, 1, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
    for q in primes[1:L + 1]:
        assert 3 * q < q0 >> 1
        vals += [q0 - q, q0 - 3 * q, q % q0]
    draw = lambda r, w: r.integers(0, q0, w, dtype=np.uint64).astype(object)  # noqa: E731
    return u64(_runs(vals, n, rng, draw, rot))


def _lift_input(e, o, level, npoly, seed):
    """(2, npoly, level + 1, n) residues whose limb 0 is the pattern; limbs above 0 are random (a
    ModRaise reads limb 0 only).  Returns the array and the coefficient-form limb 0 (2, npoly, n)."""
    n = _n(e)
    rng = np.random.default_rng(seed)
    arr = _pool(e.primes, level, 2, npoly, seed + 1, n=n)
    v = np.stack([np.stack([_lift_pattern(e.primes, e.max_level, n, rng, 3 * b + p) for p in range(npoly)])
                  for b in range(2)])
    arr[:, :, 0] = ntt_limbs(o, v.reshape(-1, n), [0] * (2 * npoly), 0).reshape(v.shape)
    return arr, v


def _check_mod_raise(e, o, cases=((0, 2), (0, 3), (2, 2))):
    """Raised to the top level, limb i is NTT_i(centre_{q0}(v) mod q_i); cases: (input level,
    polynomials)."""
    L, outs = e.max_level, []
    for level, npoly in cases:
        arr, v = _lift_input(e, o, level, npoly, 500 + 10 * level + npoly)
        r = e.mod_raise(e.import_residues(arr), L)
        assert (r.level, r.batch, r.npoly, r.is_zero) == (L, 2, npoly, False)
        want = np.stack([lift_ref(v, e.primes[0], q) for q in e.primes[:L + 1]], axis=2)
        got = e.export_residues(r)
        _eq(got, ntt_poly(o, want, 0), f"mod_raise of {npoly} polynomials from level {level}")
        outs.append(got)
    z = e.mod_raise(e.zeros(2, 0), L)
    assert (z.level, z.batch, z.npoly, z.is_zero) == (L, 2, 2, True) and not e.export_residues(z).any()
    return outs


def test_mod_raise_on_the_oracle(o12):
    L, q0 = o12.max_level, o12.primes[0]
    arr, v = _lift_input(o12, o12, 0, 2, 502)
    for i in range(1, L + 1):  # the zero-remainder negatives are there, for every target limb
        neg = obj(v[0, 0]) > (q0 >> 1)
        assert (neg & ((q0 - obj(v[0, 0])) % o12.primes[i] == 0)).sum() >= 2
    for x in ((q0 - 1) // 2, (q0 + 1) // 2):
        assert (v[0, 0] == x).any()
    outs = _check_mod_raise(o12, o12)
    wrong = np.stack([lift_ref(v, q0, q, ge=True) for q in o12.primes[:L + 1]], axis=2)
    assert not np.array_equal(ntt_poly(o12, wrong, 0), outs[0])  # centring with >= fails


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_mod_raise_gpu(w12):
    _both(_check_mod_raise, *w12)


# ------------------------------------------------------------------------------------------------
# 4. mul_i
def _check_mul_i(e, o):
    """Times +-X^{N/2} in coefficient form, both signs, 2 and 3 polynomials, the edge pool at the
    top level; (+) then (-) is the identity, (+) twice is negate."""
    l, n, outs = e.max_level, _n(e), []
    B = 2 if n <= 1 << 12 else 1
    for npoly, rots in ((2, ROTS2), (3, ROTS3)):
        arr = _edge_pool(e.primes, l, rots[:B], 600 + npoly, n=n)
        coef = ntt_poly(o, arr, 1)
        ct = e.import_residues(arr)
        for sign in (1, -1):
            want = np.stack([mul_i_ref(coef[:, :, i], q, sign) for i, q in enumerate(e.primes[:l + 1])], axis=2)
            r = e.multiply_i(ct, sign)
            assert (r.level, r.batch, r.npoly, r.is_zero) == (l, B, npoly, False)
            got = e.export_residues(r)
            _eq(got, ntt_poly(o, want, 0), f"mul_i sign {sign}, {npoly} polynomials")
            outs.append(got)
        up = e.multiply_i(ct, 1)
        _eq(e.export_residues(e.multiply_i(up, -1)), arr, "mul_i(+) then mul_i(-)")
        _eq(e.export_residues(e.multiply_i(up, 1)), e.export_residues(e.negate(ct)), "mul_i(+) twice vs negate")
    return outs


def test_mul_i_on_the_oracle(o12):
    outs = _check_mul_i(o12, o12)
    assert not np.array_equal(outs[0], outs[1])  # the sign is seen
    l = o12.max_level
    arr = _edge_pool(o12.primes, l, ROTS2, 602, n=_n(o12))
    coef = ntt_poly(o12, arr, 1)
    noneg = np.concatenate([coef[..., _n(o12) // 2:], coef[..., :_n(o12) // 2]], axis=-1)  # a cyclic shift: no sign
    assert not np.array_equal(ntt_poly(o12, noneg, 0), outs[0])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_mul_i_gpu(w12):
    _both(_check_mul_i, *w12)


# ------------------------------------------------------------------------------------------------
# 5. the automorphism
def _galois_rotations(n):
    return [1, -1, -5, n // 4 - 1, n // 4]


def _hoisted_key(e, sk, g):
    """aesfhe_key_galois_hoisted for any element (the facade makes them for rotations only)."""
    out = C.c_void_p()
    e._check(e._lib.key_galois_hoisted(e._h, sk._h, g, C.byref(out)))
    k = e._key(FixedRotationKey, out.value)
    k.galois_elt = g
    return k


def _check_galois(e, o, levels, rotations):
    """With c1 = 0 the key switch of zero is exactly zero: galois(ct, key) is (sigma_g(c0), 0), for
    the conjugation and each rotation; rotate_hoisted with the hoisted keys of the same elements
    (one call for all of them) too."""
    n, outs = _n(e), []
    B = 2 if n <= 1 << 12 else 1
    sk = e.create_secret_key(9)
    keys = [("conjugation", e.create_conjugation_key(sk))]
    keys += [(f"rotation by {d}", e.create_fixed_rotation_key(sk, d)) for d in rotations]
    hkeys = [_hoisted_key(e, sk, k.galois_elt) for _, k in keys]
    assert keys[0][1].galois_elt == 2 * n - 1 and len({k.galois_elt for _, k in keys}) == len(keys)
    for l in levels:
        arr = np.zeros((B, 2, l + 1, n), dtype=np.uint64)
        arr[:, 0] = _edge_pool(e.primes, l, [[b] for b in range(B)], 700 + l, n=n)[:, 0]
        coef = ntt_poly(o, arr[:, 0], 1)
        ct = e.import_residues(arr)
        hoisted = e.rotate_hoisted(ct, hkeys)
        for (name, key), hr in zip(keys, hoisted):
            w = np.stack([galois_ref(coef[:, i], key.galois_elt, q) for i, q in enumerate(e.primes[:l + 1])], axis=1)
            want = ntt_poly(o, w, 0)
            for how, r in (("galois", e._call_ct(e._lib.galois, ct._h, key._h)), ("rotate_hoisted", hr)):
                assert (r.level, r.batch, r.npoly) == (l, B, 2)
                got = e.export_residues(r)
                assert not got[:, 1].any(), f"{how}, {name} at level {l}: polynomial 1 is not zero"
                _eq(got[:, 0], want, f"{how}, {name} at level {l}")
                outs.append(got)
    return outs


def test_galois_on_the_oracle(o12):
    n, l = _n(o12), o12.max_level
    outs = _check_galois(o12, o12, [l], _galois_rotations(n))
    # the comparison bites: the permutation without the sign of X^{g k mod 2N}, k with g k >= N
    arr = _edge_pool(o12.primes, l, [[0], [1]], 700 + l, n=n)[:, 0]
    coef = ntt_poly(o12, arr, 1)
    g = 2 * n - 1
    idx = (g * np.arange(n)) % (2 * n) % n
    nosign = np.empty_like(coef)
    nosign[..., idx] = coef
    assert not np.array_equal(ntt_poly(o12, nosign, 0), outs[0][:, 0])
    x = np.arange(1, 9, dtype=np.uint64)  # by hand at n = 8, q = 97, g = 3: X^k -> X^{3k mod 16}
    assert galois_ref(x, 3, 97).tolist() == [1, 97 - 4, 7, 2, 97 - 5, 8, 3, 97 - 6]


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_galois_gpu(w12):
    g, o = w12
    _both(_check_galois, g, o, [g.max_level, 1], _galois_rotations(_n(g)))


# ------------------------------------------------------------------------------------------------
# 6. rescale and level-down
def _check_rescale(e, o, levels, npolys=(2, 3)):
    """rescale (C = 1) and the level-down by one level (C folded in) of _centre_ct's inputs, whose
    top limb sits on the centring boundary."""
    outs = []
    B = 2 if _n(e) <= 1 << 12 else 1
    for l in levels:
        for npoly in npolys:
            for folded in (False, True):
                arr, _ = _centre_ct(o, l, npoly, B, 900 + 10 * l + npoly, folded)
                Cc = level_down_const_ref(o.scales, o.primes, l) if folded else 1
                ct = e.import_residues(arr)
                r = e.level_down(ct, l - 1) if folded else e.rescale(ct)
                assert (r.level, r.batch, r.npoly, r.is_zero) == (l - 1, B, npoly, False)
                got = e.export_residues(r)
                _eq(got, rescale_ref(o, arr, o.primes, Cc),
                    f"{'level_down' if folded else 'rescale'} from level {l}, {npoly} polynomials")
                outs.append(got)
    return outs


def test_rescale_on_the_oracle(o12):
    L = o12.max_level
    assert {W12_CLASSES[L], W12_CLASSES[L - 1]} == {"B", "s"}  # a top prime of each class
    for l in (L, L - 1):
        assert level_down_const_ref(o12.scales, o12.primes, l) == _level_down_const(o12, l) > 1
        for folded in (False, True):  # the boundary words are in the input
            arr, want = _centre_ct(o12, l, 2, 2, 900 + 10 * l + 2, folded)
            _check_centre(o12, arr, want, l, folded)
    outs = _check_rescale(o12, o12, (L, L - 1))
    for k, folded in enumerate((False, True)):  # centring with >= fails, with and without C
        arr, _ = _centre_ct(o12, L, 2, 2, 900 + 10 * L + 2, folded)
        Cc = level_down_const_ref(o12.scales, o12.primes, L) if folded else 1
        assert not np.array_equal(rescale_ref(o12, arr, o12.primes, Cc, ge=True), outs[k])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_rescale_gpu(w12):
    g, o = w12
    _both(_check_rescale, g, o, (g.max_level, g.max_level - 1))


# ------------------------------------------------------------------------------------------------
# 7. dot_pt
DOT_PT_N = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 256)


def _dot_pt(e, cts, pts):
    n = len(cts)
    return e._call_ct(e._lib.dot_pt, (c_ct_p * max(n, 1))(*[c._h for c in cts]), (c_pt_p * max(n, 1))(*[p._h for p in pts]), n)


def _dot_operands(e, l, npoly, B):
    """Three ciphertext arrays (all-(q - 1), two edge pools) and 3 x 2 plaintexts: coefficient
    vectors [-1, 0, ...] (every residue q - 1), half INT64_MIN, seeded random +-2^62, each made at
    level l and at l + 1; the plaintexts' residues read back through add_pt."""
    n = _n(e)
    rots = [[(b + p) % 8 for p in range(npoly)] for b in range(B)]
    arrs = [_const_pool(e.primes, l, B, npoly, lambda q: q - 1, n=n), _edge_pool(e.primes, l, rots, 810, n=n),
            _edge_pool(e.primes, l, [[r + 3 for r in row] for row in rots], 811, n=n)]
    rng = np.random.default_rng(812)
    co = np.zeros((3, n), dtype=np.int64)
    co[0, 0] = -1
    co[1, :n // 2] = I64_MIN
    co[2] = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64, endpoint=True)
    pts = [[_pt_create(e, co[k], l + up) for up in (0, 1)] for k in range(3)]
    pres = [[_pt_residues(e, pts[k][up], l + up)[:l + 1] for up in (0, 1)] for k in range(3)]
    for up in (0, 1):
        assert all(int(pres[0][up][i].min()) == q - 1 for i, q in enumerate(e.primes[:l + 1]))
    return arrs, [e.import_residues(a) for a in arrs], pts, pres


def _dot_terms(ops, n):
    """Term i: ciphertext i mod 3, plaintext kind (i // 3) mod 3, every second one made a level up."""
    arrs, cts, pts, pres = ops
    ix = [(i % 3, (i // 3) % 3, i % 2) for i in range(n)]
    return ([cts[c] for c, _, _ in ix], [pts[k][u] for _, k, u in ix], [arrs[c] for c, _, _ in ix],
            [pres[k][u] for _, k, u in ix])


def _dot_expect(e, arrs, pres, l):
    """rescale(import_residues(sum ct_i pt_i mod q)), the sum in Python integers."""
    return e.export_residues(e.rescale(e.import_residues(dot_pt_sum_ref(arrs, pres, e.primes[:l + 1]))))


def _check_dot_pt(e, o, sizes, l=3):
    outs = []
    B = 2 if _n(e) <= 1 << 12 else 1
    ops = _dot_operands(e, l, 2, B)
    for n in sizes:
        cts, pts, arrs, pres = _dot_terms(ops, n)
        r = _dot_pt(e, cts, pts)
        assert (r.level, r.batch, r.npoly, r.is_zero) == (l - 1, B, 2, False)
        got = e.export_residues(r)
        _eq(got, _dot_expect(e, arrs, pres, l), f"dot_pt n = {n}")
        outs.append(got)
    return outs


def _check_dot_pt_shapes(e, o, l=3):
    """A ciphertext one level up (aligned by level-down), zero-flagged inputs, 3 polynomials, and
    the limits on n."""
    outs, n5 = [], 5
    ops = _dot_operands(e, l, 2, 2)
    cts, pts, arrs, pres = _dot_terms(ops, n5)
    hi = e.import_residues(_edge_pool(e.primes, l + 1, ROTS2, 820, n=_n(e)))
    cts2, arrs2 = list(cts), list(arrs)
    cts2[2], arrs2[2] = hi, e.export_residues(e.level_down(hi, l))
    got = e.export_residues(_dot_pt(e, cts2, pts))
    _eq(got, _dot_expect(e, arrs2, pres, l), "dot_pt with one ciphertext a level up")
    outs.append(got)
    cts3 = list(cts)
    cts3[1] = cts3[4] = e.zeros(2, l)
    keep = [0, 2, 3]
    got = e.export_residues(_dot_pt(e, cts3, pts))
    _eq(got, _dot_expect(e, [arrs[i] for i in keep], [pres[i] for i in keep], l), "dot_pt with zero-flagged inputs")
    outs.append(got)
    z = _dot_pt(e, [e.zeros(2, l)] * 3, pts[:3])
    assert (z.level, z.batch, z.npoly, z.is_zero) == (l - 1, 2, 2, True) and not e.export_residues(z).any()
    ops3 = _dot_operands(e, l, 3, 2)
    cts, pts, arrs, pres = _dot_terms(ops3, 9)
    r = _dot_pt(e, cts, pts)
    assert (r.level, r.batch, r.npoly) == (l - 1, 2, 3)
    got = e.export_residues(r)
    _eq(got, _dot_expect(e, arrs, pres, l), "dot_pt of 3-polynomial inputs")
    outs.append(got)
    for n in (0, 257):
        cts, pts, _, _ = _dot_terms(ops, n)
        with pytest.raises(RuntimeError, match="dot_pt needs 1..256 terms"):
            _dot_pt(e, cts, pts)
    return outs


def test_dot_pt_on_the_oracle(o12):
    outs = _check_dot_pt(o12, o12, DOT_PT_N)
    _check_dot_pt_shapes(o12, o12)
    # the comparison bites: the sum without its last term differs
    ops = _dot_operands(o12, 3, 2, 2)
    _, _, arrs, pres = _dot_terms(ops, 9)
    assert np.array_equal(_dot_expect(o12, arrs, pres, 3), outs[DOT_PT_N.index(9)])
    assert not np.array_equal(_dot_expect(o12, arrs[:8], pres[:8], 3), outs[DOT_PT_N.index(9)])
    assert not np.array_equal(outs[DOT_PT_N.index(8)], outs[DOT_PT_N.index(9)])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_dot_pt_gpu(w12):
    g, o = w12
    _both(_check_dot_pt, g, o, DOT_PT_N)
    _both(_check_dot_pt_shapes, g, o)


# ------------------------------------------------------------------------------------------------
# 8. the codec's ties and overflow guard
TIE_SCALE = 2.0 ** 40
TIES = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 52 - 0.5, 8.9e18, -8.9e18)


def _tie_slots(log_n, c):
    """The constant slot vector (c - i c) / scale: it encodes to c at k = 0 and -c at k = N / 2."""
    n = 1 << (log_n - 1)
    return np.full(n, c / TIE_SCALE), np.full(n, -c / TIE_SCALE)


def _tie_words(log_n, c, half_even=False):
    w = np.zeros(1 << log_n, dtype=np.int64)
    w[0], w[1 << (log_n - 1)] = round_tie(c, half_even), round_tie(-c, half_even)
    return w


def _encode_host(lib, log_n, re, im):
    co = np.empty(1 << log_n, dtype=np.int64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lib.check(lib.encode(log_n, dp(re), dp(im), re.size, TIE_SCALE, _p64(co)))
    return co


def _decode_host(lib, log_n, co):
    n = 1 << (log_n - 1)
    re, im = np.empty(n), np.empty(n)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lib.check(lib.decode(log_n, _p64(np.ascontiguousarray(co)), TIE_SCALE, dp(re), dp(im)))
    return re, im


@pytest.mark.parametrize("log_n", [14, 16])
def test_codec_ties_on_the_host_codec(oracle_lib, log_n):
    for c in TIES:
        assert c / TIE_SCALE * TIE_SCALE == c and float(round_tie(c)) in (c + 0.5, c - 0.5, c)
        _eq(_encode_host(oracle_lib, log_n, *_tie_slots(log_n, c)), _tie_words(log_n, c), f"encode of the tie {c}")
    for c in (9.1e18, -9.1e18):
        with pytest.raises(RuntimeError, match="overflows int64"):
            _encode_host(oracle_lib, log_n, *_tie_slots(log_n, c))
    # round-half-even fails on every odd tie
    assert [round_tie(c) for c in TIES[:6]] == [1, -1, 2, -2, 3, -3]
    assert [round_tie(c, half_even=True) for c in TIES[:6]] == [0, 0, 2, -2, 2, -2]
    assert round_tie(2.0 ** 52 - 0.5) == 1 << 52 and round_tie(2.0 ** 52 - 0.5, half_even=True) == 1 << 52
    assert round_tie(2.0 ** 52 - 1.5) == (1 << 52) - 1 and round_tie(2.0 ** 52 - 1.5, half_even=True) == (1 << 52) - 2
    for c in (0.5, -0.5, 2.5, -2.5):
        assert not np.array_equal(_tie_words(log_n, c, half_even=True), _encode_host(oracle_lib, log_n, *_tie_slots(log_n, c)))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("log_n", [14, 16])
def test_codec_ties_gpu(product_lib, oracle_lib, gpu_available, log_n):
    """encode_device of the tie vectors gives round-half-away words (batched: one row per tie),
    refuses |c| = 9.1e18, and decode_device of the words equals the host decode bit for bit."""
    e = Engine(_lib=product_lib, log_n=log_n, max_level=2, special_primes=2, seed=5)
    try:
        n, N, B = e.slot_count, 1 << log_n, len(TIES)
        dev = e.client_device
        sl = [_tie_slots(log_n, c) for c in TIES]
        re = torch.from_numpy(np.stack([s[0] for s in sl])).to(dev)
        im = torch.from_numpy(np.stack([s[1] for s in sl])).to(dev)
        co = torch.empty((B, N), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        e._check(e._lib.encode_device(e._h, re.data_ptr(), im.data_ptr(), B, n, n, TIE_SCALE, co.data_ptr()))
        got = co.cpu().numpy()
        for b, c in enumerate(TIES):
            _eq(got[b], _tie_words(log_n, c), f"encode_device of the tie {c}")
            _eq(got[b], _encode_host(oracle_lib, log_n, *sl[b]), f"encode_device vs the oracle's host codec, tie {c}")
            _eq(got[b], _encode_host(product_lib, log_n, *sl[b]), f"encode_device vs the product's host codec, tie {c}")
        ore = torch.empty((B, n), dtype=torch.float64, device=dev)
        oim = torch.empty((B, n), dtype=torch.float64, device=dev)
        e._check(e._lib.decode_device(e._h, co.data_ptr(), B, TIE_SCALE, ore.data_ptr(), oim.data_ptr()))
        e.synchronize()
        gr, gi = ore.cpu().numpy(), oim.cpu().numpy()
        for b, c in enumerate(TIES):
            for lib in (oracle_lib, product_lib):
                wr, wi = _decode_host(lib, log_n, got[b])
                assert np.array_equal(gr[b], wr) and np.array_equal(gi[b], wi), f"decode_device differs, tie {c}"
        for c in (9.1e18, -9.1e18):
            r1, i1 = _tie_slots(log_n, c)
            re1, im1 = torch.from_numpy(r1[None]).to(dev), torch.from_numpy(i1[None]).to(dev)
            co1 = torch.empty((1, N), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            with pytest.raises(RuntimeError, match="overflows int64"):
                e._check(e._lib.encode_device(e._h, re1.data_ptr(), im1.data_ptr(), 1, n, n, TIE_SCALE, co1.data_ptr()))
    finally:
        _drop(e)


# ------------------------------------------------------------------------------------------------
# N = 2^16 (the fused NTT passes) and N = 2^17 (R = 512)
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_coeff_residues_and_decrypt_n16_gpu(w16):
    g, o = w16
    try:
        _both(_check_coeffs_res, g, o)
        _both(_check_decrypt_secret, g, o, 1, 1)
    finally:
        _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_mod_raise_and_mul_i_n16_gpu(w16):
    g, o = w16
    try:
        _both(_check_mod_raise, g, o, cases=((0, 2), (0, 3)))
        _both(_check_mul_i, g, o)
    finally:
        _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_galois_n16_gpu(w16):
    g, o = w16
    try:
        _both(_check_galois, g, o, [1, g.max_level], _galois_rotations(_n(g)))
    finally:
        _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_rescale_and_dot_pt_n16_gpu(w16):
    g, o = w16
    try:
        _both(_check_rescale, g, o, (g.max_level,), npolys=(2,))  # the fused spread of the column pass
        _both(_check_dot_pt, g, o, (17,), l=g.max_level - 1)  # the plaintexts' upper level is the top
    finally:
        _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_galois_and_mod_raise_n17_gpu(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **W17)
    try:
        _both(_check_galois, g, o, [g.max_level], [1])
        _both(_check_mod_raise, g, o, cases=((0, 2),))
    finally:
        _drop(g, o)

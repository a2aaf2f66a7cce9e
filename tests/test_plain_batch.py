"""Batched per-element plaintexts (include/aesfhe_ext.h): Engine.encode_batch /
multiply_plain_batch, element i of the result = ct[i mod Bc] * values[i], one level down.

CPU: the oracle has no extension, so the facade runs the per-element sequence (slice, aesfhe_mul_pt
with that element's plaintext, concat); its slots are checked against the plain product and the
refused shapes raise.  GPU: the HIP engine's aesfhe_encode_device -> aesfhe_ptb_create_device ->
aesfhe_mul_ptb path is residue-exact against that sequence on the oracle."""
import ctypes as C
import json
import re

import numpy as np
import pytest

from conftest import PRODUCT_SO, ROOT
from aes_xor_fhe.fhe import Engine, PlaintextBatch


# ------------------------------------------------------------------------------------------------
# binding
def test_ext_symbols_are_the_ext_headers_and_only_the_product_has_them(oracle_lib):
    from aes_xor_fhe import _abi
    declared = sorted(set(re.findall(r"\b(aesfhe_[a-z0-9_]+)\s*\(", (ROOT / "include" / "aesfhe_ext.h").read_text())))
    assert sorted(_abi.EXT_SYMBOLS) == declared
    assert not set(_abi.EXT_SYMBOLS) & set(_abi.SYMBOLS)
    assert not oracle_lib.has_ext and not hasattr(oracle_lib, "mul_ptb")
    if not PRODUCT_SO.exists():
        import subprocess
        subprocess.run(["make", "-C", str(ROOT / "aes-fhe_amd")], check=True)
    prod = _abi.Lib(PRODUCT_SO)
    assert prod.has_ext and all(hasattr(prod, s[len("aesfhe_"):]) for s in _abi.EXT_SYMBOLS)


def test_product_without_the_extension_reads_as_rebuild(monkeypatch, oracle_lib):
    """load_product refuses a product library that lacks the extension symbols, and an engine
    that claims to be the HIP one never takes the per-element path."""
    from types import SimpleNamespace
    from aes_xor_fhe import _abi
    stale = SimpleNamespace(backend=_abi.PRODUCT_BACKEND, has_ext=False, cdll=SimpleNamespace())
    monkeypatch.setattr(_abi, "_PRODUCT", None)
    monkeypatch.setattr(_abi, "Lib", lambda path: stale)
    monkeypatch.setenv("AESFHE_LIB", str(PRODUCT_SO if PRODUCT_SO.exists() else ROOT / "README.md"))
    with pytest.raises(RuntimeError, match="rebuild it"):
        _abi.load_product()
    monkeypatch.undo()
    e = Engine(_lib=oracle_lib, log_n=10, max_level=2, special_primes=1, scale_bits=40, seed=2)
    ct = e.encrypt(np.ones((1, 4)), e.create_secret_key(1))
    pb = e.encode_batch(np.ones((1, 4)))
    monkeypatch.setattr(Engine, "on_device", property(lambda self: True))
    with pytest.raises(RuntimeError, match="rebuild it"):
        e.multiply_plain_batch(ct, pb)


# ------------------------------------------------------------------------------------------------
# CPU: slots
@pytest.fixture(scope="module")
def small(oracle_lib):
    e = Engine(_lib=oracle_lib, log_n=10, max_level=3, special_primes=2, scale_bits=40, seed=5)
    return e, e.create_secret_key(1)


def _values(rng, b, n):
    return rng.uniform(-1, 1, (b, n)) + 1j * rng.uniform(-1, 1, (b, n))


@pytest.mark.parametrize("bc,bp", [(4, 4), (4, 12), (1, 3)])
def test_multiply_plain_batch_decodes_to_the_products(small, bc, bp):
    e, sk = small
    rng = np.random.default_rng(10 * bc + bp)
    x, v = _values(rng, bc, e.slot_count), _values(rng, bp, e.slot_count)
    ct = e.encrypt(x, sk)
    pb = e.encode_batch(v)
    assert isinstance(pb, PlaintextBatch) and pb.batch == bp
    out = e.multiply_plain_batch(ct, pb)
    assert (out.batch, out.level, out.npoly) == (bp, ct.level - 1, 2)
    got = np.atleast_2d(e.decrypt(out, sk))
    want = np.stack([v[i] * x[i % bc] for i in range(bp)])
    # operands in the unit square at a 2^40 scale: encoding and encryption errors are ~1e-9
    np.testing.assert_allclose(got, want, atol=1e-6)
    # Engine.multiply dispatches on the operand type, and the residues are the same
    again = e.multiply(ct, pb)
    assert np.array_equal(e.export_residues(again), e.export_residues(out))


def test_multiply_plain_batch_short_rows_and_torch_values(small):
    """Rows shorter than slot_count are zero padded; a torch tensor on client_device is taken as
    a numpy array is."""
    import torch
    e, sk = small
    rng = np.random.default_rng(3)
    x, v = _values(rng, 2, e.slot_count), rng.uniform(-1, 1, (2, 7))
    ct = e.encrypt(x, sk)
    a = e.multiply_plain_batch(ct, e.encode_batch(v))
    b = e.multiply_plain_batch(ct, e.encode_batch(torch.from_numpy(v).to(e.client_device)))
    assert np.array_equal(e.export_residues(a), e.export_residues(b))
    want = np.zeros((2, e.slot_count), dtype=np.complex128)
    want[:, :7] = v * x[:, :7]
    np.testing.assert_allclose(np.atleast_2d(e.decrypt(a, sk)), want, atol=1e-6)


@pytest.mark.parametrize("bc,bp", [(3, 4), (8, 4)])
def test_refused_batches_raise(small, bc, bp):
    e, sk = small
    rng = np.random.default_rng(1)
    ct = e.encrypt(_values(rng, bc, e.slot_count), sk)
    with pytest.raises(RuntimeError, match="batch mismatch"):
        e.multiply_plain_batch(ct, e.encode_batch(_values(rng, bp, e.slot_count)))


def test_level_zero_input_raises_and_zero_stays_zero(small):
    e, sk = small
    rng = np.random.default_rng(2)
    pb = e.encode_batch(_values(rng, 4, e.slot_count))
    with pytest.raises(RuntimeError, match="level"):
        e.multiply_plain_batch(e.encrypt(_values(rng, 4, e.slot_count), sk, level=0), pb)
    with pytest.raises(RuntimeError, match="below"):  # plaintexts materialised below the ciphertext
        e.multiply_plain_batch(e.encrypt(_values(rng, 4, e.slot_count), sk, level=2),
                               e.encode_batch(_values(rng, 4, e.slot_count), level=1))
    z = e.multiply_plain_batch(e.zeros(2, 2), pb)
    assert z.is_zero and (z.batch, z.level) == (4, 1)
    assert not e.export_residues(z).any()


# ------------------------------------------------------------------------------------------------
# GPU: residues
_PAIRS = {}


def _pair(product_lib, oracle_lib, log_n):
    """The HIP engine and the oracle with the same parameters and keys (built once per ring)."""
    if log_n not in _PAIRS:
        kw = dict(log_n=log_n, max_level=6, special_primes=2, scale_bits=40, seed=17)
        pair = []
        for lib in (product_lib, oracle_lib):
            e = Engine(_lib=lib, **kw)
            pair.append((e, e.create_secret_key(1)))
        _PAIRS[log_n] = pair
    return _PAIRS[log_n]


def _profiled(eng, fn):
    eng._check(eng._lib.engine_profile(eng._h, -1))
    try:
        res = fn()
        need = C.c_int64()
        eng._check(eng._lib.engine_profile_kernels(eng._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        eng._check(eng._lib.engine_profile_kernels(eng._h, buf, need.value, C.byref(need)))
    finally:
        eng._check(eng._lib.engine_profile(eng._h, 0))
    return res, json.loads(buf.value.decode())


def _both(pair, make_ct, make_pb, expect):
    """The product on both engines from identical inputs; the HIP one under the launch profile.
    Returns the residues (equal) after the common checks."""
    res = []
    for k, (e, sk) in enumerate(pair):
        e._nonce = 1000  # the same encryption randomness on both sides
        ct, pb = make_ct(e, sk), make_pb(e)
        if k == 0:
            out, prof = _profiled(e, lambda: e.multiply_plain_batch(ct, pb))
            # the product ran the extension's kernels, not the per-element sequence
            assert prof.get("mul_ptb", [0])[0] == 1 and prof.get("ptb_create", [0])[0] == 1, prof
        else:
            out = e.multiply_plain_batch(ct, pb)
        assert (out.batch, out.level, out.npoly) == expect, out
        res.append(e.export_residues(out))
    assert np.array_equal(res[0], res[1]), "aesfhe_mul_ptb differs from the oracle's per-element aesfhe_mul_pt"
    return res[0]


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 16])
@pytest.mark.parametrize("bc,bp", [(4, 8), (8, 8)])
def test_mul_ptb_residue_exact_top_level(product_lib, oracle_lib, gpu_available, log_n, bc, bp):
    pair = _pair(product_lib, oracle_lib, log_n)
    rng = np.random.default_rng(log_n + bc)
    n = pair[0][0].slot_count
    x, v = _values(rng, bc, n), _values(rng, bp, n)
    _both(pair, lambda e, sk: e.encrypt(x, sk, level=6), lambda e: e.encode_batch(v), (bp, 5, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 16])
@pytest.mark.parametrize("bc,bp", [(4, 8), (8, 8)])
def test_mul_ptb_residue_exact_low_ciphertext_higher_plaintext(product_lib, oracle_lib, gpu_available, log_n, bc, bp):
    """Ciphertext at level 1 (the lowest legal one), plaintexts materialised at level 3: the
    plaintext's limb stride differs from the ciphertext's."""
    pair = _pair(product_lib, oracle_lib, log_n)
    rng = np.random.default_rng(2 * log_n + bc)
    n = pair[0][0].slot_count
    x, v = _values(rng, bc, n), _values(rng, bp, n)
    _both(pair, lambda e, sk: e.encrypt(x, sk, level=1), lambda e: e.encode_batch(v, level=3), (bp, 0, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 16])
def test_mul_ptb_residue_exact_three_polynomials(product_lib, oracle_lib, gpu_available, log_n):
    """A tensor output (3 polynomials, not relinearised) as the ciphertext operand."""
    pair = _pair(product_lib, oracle_lib, log_n)
    rng = np.random.default_rng(3 * log_n)
    n = pair[0][0].slot_count
    x, y, v = _values(rng, 4, n), _values(rng, 4, n), _values(rng, 8, n)

    def tensor(e, sk):
        a, b = e.encrypt(x, sk, level=4), e.encrypt(y, sk, level=4)  # held until the call returns
        t = e._call_ct(e._lib.tensor, a._h, b._h)
        assert t.npoly == 3
        return t
    _both(pair, tensor, lambda e: e.encode_batch(v), (8, 3, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 16])
def test_mul_ptb_residue_exact_extreme_coefficients(product_lib, oracle_lib, gpu_available, log_n):
    """Plaintext coefficients up to +-2^62 through the direct coefficient buffer
    (Engine.coeff_batch): the signed reduction mod q at the top of its range."""
    pair = _pair(product_lib, oracle_lib, log_n)
    rng = np.random.default_rng(5 * log_n)
    n = pair[0][0].slot_count
    x = _values(rng, 4, n)
    co = rng.integers(-2 ** 62, 2 ** 62, (8, 2 * n), dtype=np.int64, endpoint=True)
    co[:, 0], co[:, 1], co[:, 2], co[:, 3] = 2 ** 62, -2 ** 62, 0, -1
    _both(pair, lambda e, sk: e.encrypt(x, sk, level=2), lambda e: e.coeff_batch(co, level=2), (8, 1, 2))

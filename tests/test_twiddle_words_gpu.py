"""Residue parity of every kernel that reads the twiddle tables as exact words w.

The fp64 passes (csrc/ntt256f.h, ks_fused.h, bconv_cols.h) read Tabs::psid / ipsid / rtwd / irtwd
-- w itself, not w / q -- and take the modular product's quotient from the product (kernels.h
fmul_remq).  Here each of them runs once at the smallest shapes it still takes, residue for residue
against the CPU oracle (np.array_equal on export_residues, no tolerance), on a short chain whose
primes lie just below 2^42, just above it (the other fold schedule) and near 2^50, on worst-case
words: every residue q - 1, and 0 / q - 1 alternating along rows and along columns of the
256-wide NTT tile.  The launch profile is checked, so that the unfused path cannot pass for the
fused one.
"""
import ctypes as C

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine

from _ks_helpers import N16, _drop, _keys, _pair, _profiled  # noqa: E402

BIG = 1 << 42  # kernels.h kBigPrime
# scale 42: q_1.. straddle 2^42, q_0 and the special primes are 50-bit (test_range_bounds.py S42)
KW16 = dict(log_n=16, max_level=5, special_primes=4, digit_primes=4, scale_bits=42, seed=77)
KW17 = dict(log_n=17, max_level=3, special_primes=2, scale_bits=42, seed=78)
B = 2
FUSED_LABELS = ("ks_rows_fin.prod", "ks_rows_inner.prod", "ks_rows_fin.ks", "modup_cols", "moddown_cols",
                "ntt_inv_cols", "ntt_inv_rows_prod")


def _patterns(q, n):
    """(3, n): every word q - 1; 0 / q - 1 alternating along a row (neighbouring coefficients);
    the same along a column (neighbouring rows of 256)."""
    k = np.arange(n)
    out = np.zeros((3, n), dtype=np.uint64)
    out[0] = q - 1
    out[1, k % 2 == 1] = q - 1
    out[2, (k // 256) % 2 == 1] = q - 1
    return out


def _worst_ct(primes, l, n, shift):
    """(B, 2, l + 1, n) residues: (batch b, poly p) holds pattern (b + p + shift) % 3 of every limb."""
    out = np.empty((B, 2, l + 1, n), dtype=np.uint64)
    for i in range(l + 1):
        pat = _patterns(primes[i], n)
        for b in range(B):
            for p in range(2):
                out[b, p, i] = pat[(b + p + shift) % 3]
    return out


def _ntt_all(eng, limbs, inverse):
    buf = limbs.copy()
    pids = np.arange(len(limbs), dtype=np.int32)
    eng._check(eng._lib.ntt_host(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), len(limbs),
                                 pids.ctypes.data_as(C.POINTER(C.c_int32)), inverse))
    return buf


def _same(g, o, cg, co, what):
    assert (cg.level, cg.batch, cg.npoly) == (co.level, co.batch, co.npoly), f"{what}: {cg!r} vs {co!r}"
    a, b = g.export_residues(cg), o.export_residues(co)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} residues differ; first at "
                             f"[batch, poly, limb, coeff] = {bad[0].tolist()}")


@pytest.fixture(scope="module")
def pair16(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **KW16)
    st = dict(g=g, o=o, kg=_keys(g), ko=_keys(o), prof={})
    yield st
    st.clear()
    _drop(g, o)


@pytest.mark.gpu
def test_chain_has_the_three_prime_classes(pair16):
    q = pair16["g"].primes
    L = KW16["max_level"]
    assert any(p < BIG for p in q[1:L + 1]) and any(BIG <= p < 2 * BIG for p in q[1:L + 1])
    assert q[0] > 1 << 49 and all(p > 1 << 49 for p in q[L + 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
def test_ntt_worst_case_words_n16(pair16, inverse):
    g, o = pair16["g"], pair16["o"]
    for k, name in enumerate(("all q-1", "alternating along rows", "alternating along columns")):
        limbs = np.stack([_patterns(q, N16)[k] for q in g.primes])
        a, b = _ntt_all(g, limbs, inverse), _ntt_all(o, limbs, inverse)
        bad = np.argwhere(a != b)
        assert not len(bad), f"ntt_host {name} inverse={inverse}: {len(bad)} differ, first at [prime, coeff] = {bad[0].tolist()}"


@pytest.mark.gpu
def test_product_relinearised_and_rescaled_n16(pair16):
    g, o, l = pair16["g"], pair16["o"], KW16["max_level"]
    x, y = _worst_ct(g.primes, l, N16, 0), _worst_ct(g.primes, l, N16, 1)

    def run(e, k):
        out = e.multiply(e.import_residues(x), e.import_residues(y), k["rlk"])
        out._h  # the product is deferred: evaluate it here
        return out

    cg, prof = _profiled(g, lambda: run(g, pair16["kg"]))
    pair16["prof"]["multiply"] = prof
    assert cg.level == l - 1
    _same(g, o, cg, run(o, pair16["ko"]), "multiply at N = 2^16")


@pytest.mark.gpu
def test_rotate_n16(pair16):
    g, o, l = pair16["g"], pair16["o"], KW16["max_level"]
    x = _worst_ct(g.primes, l, N16, 2)
    cg, prof = _profiled(g, lambda: g.rotate(g.import_residues(x), pair16["kg"]["rot"]))
    pair16["prof"]["rotate"] = prof
    _same(g, o, cg, o.rotate(o.import_residues(x), pair16["ko"]["rot"]), "rotate at N = 2^16")


@pytest.mark.gpu
def test_the_fused_kernels_ran_n16(pair16):
    """The two ops above went through the kernels this file is about."""
    prof = pair16["prof"]
    assert set(prof) == {"multiply", "rotate"}, "run the whole module: this test reads the profiles of the two ops"
    for label in FUSED_LABELS:
        assert any(p.get(label, 0) > 0 for p in prof.values()), f"{label} did not run: {prof}"
    assert not any(p.get("ntt_generic", 0) for p in prof.values()), prof


@pytest.mark.gpu
def test_product_n17(product_lib, oracle_lib, gpu_available):
    """R = 512 instantiates the same headers."""
    g, o = _pair(product_lib, oracle_lib, **KW17)
    try:
        l, n = KW17["max_level"], 1 << 17
        assert any(p < BIG for p in g.primes[1:l + 1]) and g.primes[0] > 1 << 49
        x, y = _worst_ct(g.primes, l, n, 0), _worst_ct(g.primes, l, n, 1)
        outs = []
        for e in (g, o):
            rlk = e.create_relinearization_key(e.create_secret_key(9))
            out = e.multiply(e.import_residues(x), e.import_residues(y), rlk)
            out._h
            outs.append(out)
        _same(g, o, outs[0], outs[1], "multiply at N = 2^17")
        del outs
    finally:
        _drop(g, o)

"""Refused calls leave nothing behind.  A switching key trimmed to one digit (aesfhe_key_trim)
cannot switch where more digits are read: every entry point that key-switches must refuse with
AESFHE_ELEVEL ("key trimmed to 1 digits ..."), on the CPU oracle and on the HIP engine alike, and
on the HIP engine give back every device block it had taken by then (the engine's temporaries are
owning handles): the pool's live bytes return to their baseline, and a
permitted product afterwards is residue-identical to the oracle's."""
import gc

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine

# digits of 2 primes (digit_primes = special_primes): the top level 4 reads 3 digits, a key trimmed
# to level 1 keeps one
CHAIN = dict(max_level=4, special_primes=2, digit_primes=2, seed=23)


def _setup(lib, log_n, batch):
    e = Engine(_lib=lib, log_n=log_n, **CHAIN)
    assert e.dnum >= 3
    sk = e.create_secret_key(2)
    s = dict(e=e, sk=sk, pk=e.create_public_key(sk), rlk=e.create_relinearization_key(sk),
             gk=e.create_fixed_rotation_key(sk, 1), hk=e.create_hoisted_rotation_key(sk, 1))
    for k in ("rlk", "gk", "hk"):
        e.trim_key(s[k], 1)
    rng = np.random.default_rng(4)
    z = np.exp(2j * np.pi * rng.integers(0, 16, (3, batch, e.slot_count)) / 16)
    s["z"] = z
    s["a"], s["b"], s["c"] = (e.encrypt(z[i] if batch > 1 else z[i, 0], s["pk"]) for i in range(3))
    s["low"] = e.encrypt(z[0] if batch > 1 else z[0, 0], s["pk"], level=1)  # where one digit suffices
    s["one"] = e.encrypt(z[1, 0], s["pk"])  # batch 1: the batched power basis of the fused engines
    return s


def _refused(s):
    """(name, call) for every key-switching entry point at the top level; deferred products are
    forced by export_residues."""
    e, a, b, c, rlk = s["e"], s["a"], s["b"], s["c"], s["rlk"]
    return [
        ("rotate", lambda: e.rotate(a, s["gk"])),
        ("rotate_hoisted", lambda: e.rotate_hoisted(a, [s["hk"]])),
        ("relinearize", lambda: e.relinearize(e._call_ct(e._lib.tensor, a._h, b._h), rlk)),
        ("multiply", lambda: e.export_residues(e.multiply(a, b, rlk))),
        ("multiply_fma", lambda: e.export_residues(e.multiply_fma(a, b, rlk, 1, c, 1.0, 0.5))),
        ("dot", lambda: e.export_residues(e.dot([a, b], [b, c], rlk))),
        ("dot_fma", lambda: e.export_residues(e.dot_fma([a, b], [b, c], rlk, [(c, 1.0)], 0.5))),
        ("poly2_int", lambda: e.poly2_int([a], [b], [[[1, 2], [3, 4]], [[0, 1], [1, 0]]], 8, rlk)),
        ("make_power_basis", lambda: e.make_power_basis(a, 3, rlk)),
        ("make_power_basis of one", lambda: e.make_power_basis(s["one"], 3, rlk)),
    ]


def _refuse_all(s):
    for name, call in _refused(s):
        with pytest.raises(RuntimeError, match="trimmed"):
            call()
            pytest.fail(f"{name} was not refused")


def test_trimmed_key_refusals_oracle(oracle_lib):
    s = _setup(oracle_lib, 12, 1)
    e = s["e"]
    _refuse_all(s)
    m = e.multiply(s["low"], s["low"], s["rlk"])
    np.testing.assert_allclose(e.decrypt(m, s["sk"]), s["z"][0, 0] ** 2, atol=1e-4)


def _leak_check(product_lib, oracle_lib, log_n):
    s, o = _setup(product_lib, log_n, 2), _setup(oracle_lib, log_n, 2)
    e = s["e"]
    assert e.dnum == o["e"].dnum >= 3
    w = e.multiply(s["low"], s["low"], s["rlk"])  # anything materialised on first use exists before the baseline
    want = o["e"].export_residues(o["e"].multiply(o["low"], o["low"], o["rlk"]))
    assert np.array_equal(e.export_residues(w), want)
    del w
    gc.collect()
    e.synchronize()
    base = e.pool_stats()["live"]
    _refuse_all(s)
    gc.collect()
    e.synchronize()
    live = e.pool_stats()["live"]
    print(f"log_n={log_n}: live {live} after the refused calls, baseline {base}")
    assert live == base, (live, base)
    assert np.array_equal(e.export_residues(e.multiply(s["low"], s["low"], s["rlk"])), want)


@pytest.mark.gpu
def test_trimmed_key_refusals_leave_no_block_generic_gpu(product_lib, oracle_lib, gpu_available):
    """The generic NTT path (N = 2^12): relin_ct, the unfused mul_ct, ks_apply with an own accumulator."""
    _leak_check(product_lib, oracle_lib, 12)


@pytest.mark.gpu
def test_trimmed_key_refusals_leave_no_block_fused_gpu(product_lib, oracle_lib, gpu_available):
    """The fused paths (N = 2^16): keyswitch_prod, ks_finish_fused, the batched power basis; the
    smallest chain whose top level reads 3 digits while one digit still multiplies (level 1)."""
    _leak_check(product_lib, oracle_lib, 16)

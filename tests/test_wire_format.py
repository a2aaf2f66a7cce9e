"""The compact wire format: packed residue rows and masks expanded from a public
seed, for keys and ciphertexts (Engine.pack_key / pack_ciphertext / unpack, save(compact=True),
aes_xor_fhe.wire).

CPU, on the oracle (the facade's numpy / Python-integer path): round trips word for word against
aesfhe_key_export / aesfhe_ct_export, the payload against a packer written here in Python integers,
the seeded masks against a ChaCha20 block function written here (pinned to RFC 7539's block
vector), the re-masking identity b' + a' s = b + a s at every index in Python integers, the
operations under unpacked seeded keys, every refusal, and the header parser / host row codec under
ASan + UBSan (tests/native/wire_format_asan.cpp).  GPU: the HIP engine's blobs are byte-identical to
that path's, its refusals leave the pool as it was, one launch per direction, and a reduced CTR
pipeline runs under keys that went through save_evaluation_keys.

Chains: L = 4, K = 2 with digits of 2 primes (3 digits) and of 3 primes (2 digits, the last one
short).  A digit of 3 primes must stay below P = two 50-bit primes (digits_below_p), so that chain
takes a 36-bit base prime and a 31-bit scale; its rows then pack to 36, 31 and 32 bits (below 32
bits a packed word draws on more than three residues), the other chain's to 50, 40 and 41."""
import ctypes as C
import functools
import gc
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from aes_xor_fhe import aes_tables as T
from aes_xor_fhe import wire
from aes_xor_fhe.aes_round_bits import AESSlicedRound
from aes_xor_fhe.fhe import (ConjugationKey, Engine, FixedRotationKey, GaloisKey, PublicKey, RelinearizationKey,
                             SecretKey)
from conftest import ROOT

CHAINS = {"A2": dict(max_level=4, special_primes=2, digit_primes=2, scale_bits=40),
          "A3": dict(max_level=4, special_primes=2, digit_primes=3, scale_bits=31, base_bits=36)}
SEED = bytes(range(100, 132))
SEED2 = bytes(range(7, 39))
M64 = (1 << 64) - 1
TAG, CT_KIND = 0x57495245464D5431, 0xC7


# ------------------------------------------------------------------------------------------------
# the format restated in Python integers (nothing here calls aes_xor_fhe.wire)
def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _derive(a, b):
    return _mix64(a ^ _mix64(b))


def _label(kind, galois, index):
    return _derive(_derive(_derive(TAG, kind), galois), index)


def _chacha_block(key, w12, w13, w14, w15):
    """RFC 7539 section 2.3: 8 key words and the last four state words -> 16 output words."""
    rotl = lambda x, n: ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF
    x = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key, w12, w13, w14, w15]
    w = list(x)

    def qr(a, b, c, d):
        w[a] = (w[a] + w[b]) & 0xFFFFFFFF; w[d] = rotl(w[d] ^ w[a], 16)
        w[c] = (w[c] + w[d]) & 0xFFFFFFFF; w[b] = rotl(w[b] ^ w[c], 12)
        w[a] = (w[a] + w[b]) & 0xFFFFFFFF; w[d] = rotl(w[d] ^ w[a], 8)
        w[c] = (w[c] + w[d]) & 0xFFFFFFFF; w[b] = rotl(w[b] ^ w[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return [(a + b) & 0xFFFFFFFF for a, b in zip(w, x)]


def _mask_row(seed, lab, pid, log_n, q):
    """The mask row of prime pid: block ((pid << log_n) + k0) >> 3 of the stream keyed by the seed
    bytes gives residues k0 .. k0 + 7, each floor(word64 * q / 2^64)."""
    key = struct.unpack("<8I", seed)
    out = []
    for k0 in range(0, 1 << log_n, 8):
        ctr = ((pid << log_n) + k0) >> 3
        o = _chacha_block(key, ctr & 0xFFFFFFFF, ctr >> 32, lab & 0xFFFFFFFF, lab >> 32)
        out += [((o[2 * i] | (o[2 * i + 1] << 32)) * q) >> 64 for i in range(8)]
    return out


def _pack_rows_int(rows, primes):
    """rows: (limb, residues) in blob order -> payload bytes, each row one big little-endian integer."""
    out = b""
    for l, res in rows:
        w = (primes[l] - 1).bit_length()
        out += sum(int(v) << (k * w) for k, v in enumerate(res)).to_bytes(len(res) * w // 8, "little")
    return out


def _size(e, groups, polys, nl):
    return 128 + groups * polys * sum((q - 1).bit_length() for q in e.primes[:nl]) * (1 << e.log_coeff_count) // 8


def _brv(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2)


def _galois_rows(rows, g, log_n):
    """X -> X^g on NTT rows: out[k] = in[brv((g (2 brv(k) + 1) mod 2N - 1) / 2)]."""
    n = 1 << log_n
    idx = [_brv(((g * (2 * _brv(k, log_n) + 1)) % (2 * n) - 1) // 2, log_n) for k in range(n)]
    return rows[..., idx]


def test_chacha_block_rfc7539_vector():
    key = struct.unpack("<8I", bytes(range(32)))
    want = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
            0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    assert _chacha_block(key, 1, 0x09000000, 0x4a000000, 0) == want
    # and the package's vectorised one, same vector: counter words (1, 0x09000000), label words after
    got = wire.chacha_blocks(key, 0x4a000000, np.array([1 | (0x09000000 << 32)], dtype=np.uint64))
    assert got[0].tolist() == want


# ------------------------------------------------------------------------------------------------
# objects
@functools.lru_cache(maxsize=None)
def _objs(lib, log_n, chain, engine_seed=23):
    e = Engine(_lib=lib, log_n=log_n, seed=engine_seed, **CHAINS[chain])
    sk, sk2 = e.create_secret_key(2), e.create_secret_key(9)
    pk = e.create_public_key(sk)
    o = dict(e=e, sk=sk, sk2=sk2, pk=pk)
    # name -> (key, the secret its rows are encrypted under)
    o["keys"] = {
        "public": (pk, sk),
        "relin": (e.create_relinearization_key(sk), sk),
        "galois": (e.create_fixed_rotation_key(sk, 1), sk),
        "galois2": (e.create_fixed_rotation_key(sk, 2), sk),
        "conj": (e.create_conjugation_key(sk), sk),
        "hoisted": (e.create_hoisted_rotation_key(sk, 3), sk),
        "switch": (e.create_switching_key(sk, sk2), sk2),
        "trimmed": (e.trim_key(e.create_relinearization_key(sk), 1), sk),
    }
    rng = np.random.default_rng(4)
    z = np.exp(2j * np.pi * rng.integers(0, 16, (2, 3, e.slot_count)) / 16)
    o["z"] = z
    e._nonce = 500
    o["ct2"] = e.encrypt(z[0], pk)
    b = e.encrypt(z[1], pk)
    o["ct3"] = e._call_ct(e._lib.tensor, o["ct2"]._h, b._h)
    o["ctb"] = b
    return o


def _export(e, k):
    return wire.export_key(e, k)


def _rows_of(e, kind, data):
    n = 1 << e.log_coeff_count
    Lp1, n_p = e.max_level + 1, e.max_level + 1 + e.special_prime_count
    return data.reshape({0: (1, 1, n_p, n), 1: (1, 2, Lp1, n)}.get(kind, (-1, 2, n_p, n)))


CASES = [(10, "A2"), (10, "A3"), (11, "A2"), (11, "A3")]


# ------------------------------------------------------------------------------------------------
# 1. round trip without a seed
@pytest.mark.parametrize("log_n,chain", CASES)
def test_round_trip_unseeded(oracle_lib, log_n, chain):
    o = _objs(oracle_lib, log_n, chain)
    e = o["e"]
    assert e.dnum == (3 if chain == "A2" else 2)
    keys = dict(o["keys"], secret=(o["sk"], None))
    for name, (k, _) in keys.items():
        kind, g, ks, data = _export(e, k)
        rows = _rows_of(e, kind, data)
        blob = e.pack_key(k)
        assert len(blob) == _size(e, *rows.shape[:3]) == wire.blob_bytes(e, kind, rows.shape[0]), name
        k2 = e.unpack(blob)
        kind2, g2, ks2, data2 = _export(e, k2)
        assert (kind2, g2, ks2) == (kind, g, ks) and np.array_equal(data2, data), name
        assert type(k2) is type(k), (name, type(k2))  # the class follows the kind and the galois element
        if isinstance(k, FixedRotationKey):
            assert k2.delta % e.slot_count == k.delta % e.slot_count and k2.galois_elt == k.galois_elt
    assert _rows_of(e, 2, _export(e, keys["trimmed"][0])[3]).shape[0] == 1 < e.dnum
    for name in ("ct2", "ct3"):
        c = o[name]
        blob = e.pack_ciphertext(c)
        assert len(blob) == _size(e, 3, c.npoly, c.level + 1) == wire.blob_bytes(e, batch=3, npoly=c.npoly, level=c.level)
        c2 = e.unpack(blob)
        assert (c2.batch, c2.npoly, c2.level, c2.is_zero) == (3, c.npoly, c.level, False)
        assert np.array_equal(e.export_residues(c2), e.export_residues(c)), name
    low = e.level_down(o["ct2"], 2)  # fewer limbs than the chain
    assert np.array_equal(e.export_residues(e.unpack(e.pack_ciphertext(low))), e.export_residues(low))


# ------------------------------------------------------------------------------------------------
# 2. packing against a second implementation
@pytest.mark.parametrize("log_n,chain", [(10, "A2"), (10, "A3")])
def test_payload_against_python_integer_packer(oracle_lib, log_n, chain):
    o = _objs(oracle_lib, log_n, chain)
    e = o["e"]
    for name in ("galois", "public", "trimmed"):
        kind, _, _, data = _export(e, o["keys"][name][0])
        rows = _rows_of(e, kind, data)
        order = [(l, rows[g, p, l]) for g in range(rows.shape[0]) for p in range(rows.shape[1]) for l in range(rows.shape[2])]
        assert e.pack_key(o["keys"][name][0])[128:] == _pack_rows_int(order, e.primes), name
    res = e.export_residues(o["ct3"])
    order = [(l, res[b, p, l]) for b in range(3) for p in range(3) for l in range(res.shape[2])]
    blob = e.pack_ciphertext(o["ct3"])
    assert blob[128:] == _pack_rows_int(order, e.primes)
    # one flipped payload bit changes exactly one residue: bit 2 of residue 5 of row (0, 1, 1)
    n, w0, w1 = 1 << log_n, (e.primes[0] - 1).bit_length(), (e.primes[1] - 1).bit_length()
    wsum = sum((q - 1).bit_length() for q in e.primes[:res.shape[2]])
    bit = 128 * 8 + (1 * wsum + w0) * n + 5 * w1 + 2
    assert (int(res[0, 1, 1, 5]) ^ 4) < e.primes[1]
    bad = bytearray(blob)
    bad[bit // 8] ^= 1 << (bit % 8)
    got = e.export_residues(e.unpack(bytes(bad)))
    diff = np.argwhere(got != res)
    assert diff.tolist() == [[0, 1, 1, 5]] and int(got[0, 1, 1, 5]) == int(res[0, 1, 1, 5]) ^ 4
    # a residue forced to q is refused: residue 7 of row (2, 0, 1)
    forced = res.copy()
    forced[2, 0, 1, 7] = e.primes[1]
    order = [(l, forced[b, p, l]) for b in range(3) for p in range(3) for l in range(res.shape[2])]
    with pytest.raises(RuntimeError, match="invalid argument.*not below its prime"):
        e.unpack(blob[:128] + _pack_rows_int(order, e.primes))


# ------------------------------------------------------------------------------------------------
# 3. seeded packing
def _seeded_rows(e, blob):
    """(header fields, b' rows (groups, nl, N), a' rows) of a seeded blob through Engine.unpack."""
    f = wire.header_fields(blob)
    obj = e.unpack(blob)
    if f["type"] == wire.TYPE_CT:
        rows = e.export_residues(obj)
    else:
        kind, _, _, data = _export(e, obj)
        rows = _rows_of(e, kind, data)
    return f, rows[:, 0].astype(object), rows[:, 1].astype(object)


def _check_identity(e, orig, bp, ap, s, holds=True):
    """b' + a' s == b + a s mod every prime at every index (or, holds=False, somewhere not)."""
    same = True
    for l in range(orig.shape[2]):
        q = e.primes[l]
        lhs = (bp[:, l] + ap[:, l] * s[l]) % q
        rhs = (orig[:, 0, l].astype(object) + orig[:, 1, l].astype(object) * s[l]) % q
        same = same and bool((lhs == rhs).all())
    assert same == holds


@pytest.mark.parametrize("log_n,chain", CASES)
def test_seeded_masks_and_identity(oracle_lib, log_n, chain):
    o = _objs(oracle_lib, log_n, chain)
    e = o["e"]
    n = 1 << log_n
    sres = {id(o["sk"]): _export(e, o["sk"])[3].reshape(-1, n), id(o["sk2"]): _export(e, o["sk2"])[3].reshape(-1, n)}
    masks = {}
    for name, (k, target) in o["keys"].items():
        kind, g, ks, data = _export(e, k)
        orig = _rows_of(e, kind, data)
        blob = e.pack_key(k, target, SEED)
        assert blob == e.pack_key(k, target, SEED), name  # the same seed gives the same bytes
        assert len(blob) == _size(e, orig.shape[0], 1, orig.shape[2]) == wire.blob_bytes(e, kind, orig.shape[0], seeded=True)
        f, bp, ap = _seeded_rows(e, blob)
        assert (f["seeded"], f["seed"], f["kind"], f["galois"], f["keyseed"], f["ndig"]) == \
            (1, SEED, kind, g, ks, orig.shape[0] if kind >= 2 else 0), name
        # the masks: every row at N = 2^10, the first and last limb of every digit above
        for d in range(orig.shape[0]):
            for l in (range(orig.shape[2]) if log_n == 10 else (0, orig.shape[2] - 1)):
                assert ap[d, l].tolist() == _mask_row(SEED, _label(kind, g, d), l, log_n, e.primes[l]), (name, d, l)
        masks[name] = ap
        s = sres[id(target)].astype(object)
        if kind == 5:
            s = _galois_rows(s, pow(g, -1, 2 * n), log_n)
        _check_identity(e, orig, bp, ap, s)
        wrong = sres[id(o["sk2"] if target is o["sk"] else o["sk"])].astype(object)
        _check_identity(e, orig, bp, ap, wrong, holds=False)
    # a wrong target_sk at packing time breaks it too
    kind, g, _, data = _export(e, o["keys"]["galois"][0])
    _, bp, ap = _seeded_rows(e, e.pack_key(o["keys"]["galois"][0], o["sk2"], SEED))
    _check_identity(e, _rows_of(e, kind, data), bp, ap, sres[id(o["sk"])].astype(object), holds=False)
    # two galois elements, two digits, two seeds: different masks
    assert not (masks["galois"][0, 0] == masks["galois2"][0, 0]).any() or n < 8
    assert (masks["galois"][0, 0] != masks["galois2"][0, 0]).sum() > n - 8
    assert (masks["galois"][0, 0] != masks["galois"][1, 0]).sum() > n - 8
    _, _, other = _seeded_rows(e, e.pack_key(o["keys"]["galois"][0], o["sk"], SEED2))
    assert (masks["galois"][0, 0] != other[0, 0]).sum() > n - 8
    # ciphertexts: encrypted under the public key (batch 3) and the label of each batch element
    res = e.export_residues(o["ct2"])
    blob = e.pack_ciphertext(o["ct2"], o["sk"], SEED)
    assert len(blob) == _size(e, 3, 1, o["ct2"].level + 1) and blob == e.pack_ciphertext(o["ct2"], o["sk"], SEED)
    f, bp, ap = _seeded_rows(e, blob)
    assert (f["batch"], f["npoly"], f["level"], f["seeded"]) == (3, 2, o["ct2"].level, 1)
    for b in range(3):
        for l in (0, res.shape[2] - 1):
            assert ap[b, l].tolist() == _mask_row(SEED, _label(CT_KIND, 0, b), l, log_n, e.primes[l])
    _check_identity(e, res, bp, ap, sres[id(o["sk"])].astype(object))
    np.testing.assert_allclose(e.decrypt(e.unpack(blob), o["sk"]), o["z"][0], atol=1e-4 if chain == "A2" else 1e-2)
    # os.urandom seeds: two packs differ, both unpack to the same plaintext
    r1, r2 = e.pack_ciphertext(o["ct2"], o["sk"]), e.pack_ciphertext(o["ct2"], o["sk"])
    assert r1 != r2 and len(r1) == len(blob)


# ------------------------------------------------------------------------------------------------
# 4. function: operations under unpacked seeded keys
def _decrypt_coeffs(e, ct, sk):
    co = np.empty((ct.batch, 1 << e.log_coeff_count), dtype=np.int64)
    e._check(e._lib.decrypt(e._h, sk._h, ct._h, co.ctypes.data_as(C.POINTER(C.c_int64))))
    return co


def test_operations_under_seeded_keys(oracle_lib):
    """Against the plain result, the maximum deviation under unpacked seeded keys is at most 4 times
    the one under the original keys (the same error polynomial under another mask sample; 4 covers
    the spread of a maximum over so few slots).  Exactness is test_seeded_masks_and_identity's."""
    o = _objs(oracle_lib, 11, "A2")
    e, sk, z = o["e"], o["sk"], o["z"]
    seeded = {name: e.unpack(e.pack_key(k, t, SEED)) for name, (k, t) in o["keys"].items()}
    orig = {name: k for name, (k, _) in o["keys"].items()}
    a, b = o["ct2"], o["ctb"]

    def dev(ct, want):
        return float(np.abs(e.decrypt(ct, sk) - want).max())

    ops = {
        "rotate": (lambda K: e.rotate(a, K["galois"]), np.roll(z[0], 1, axis=1)),
        "relinearise": (lambda K: e.rescale(e.relinearize(e._call_ct(e._lib.tensor, a._h, b._h), K["relin"])), z[0] * z[1]),
        "rotate_hoisted": (lambda K: e.rotate_hoisted(a, [K["hoisted"]])[0], np.roll(z[0], 3, axis=1)),
    }
    for name, (op, want) in ops.items():
        d0, d1 = dev(op(orig), want), dev(op(seeded), want)
        print(f"{name}: deviation {d0:.3e} with the original key, {d1:.3e} with the seeded one")
        assert 0 < d1 <= 4 * d0, name
    # one expand step, in coefficients: element t holds the coefficients 2 w + t at index 2 w
    xk = e.create_expansion_keys(sk, 0, 1)
    xs = [e.unpack(e.pack_key(xk[0], sk, SEED))]
    rng = np.random.default_rng(1)
    co = rng.integers(-2 ** 30, 2 ** 30, 1 << 11) << 10
    want = np.zeros((2, 1 << 11), dtype=np.int64)
    want[0, 0::2], want[1, 0::2] = co[0::2], co[1::2]
    e._nonce = 900
    c = e.encrypt_coefficients(co, o["pk"], 3)
    d0 = np.abs(_decrypt_coeffs(e, e.expand(c, xk), sk) - want).max()
    d1 = np.abs(_decrypt_coeffs(e, e.expand(c, xs), sk) - want).max()
    print(f"expand step: deviation {d0} / {d1}")
    assert 0 < d1 <= 4 * d0


def test_seeded_bundle_through_expand_round_keys(oracle_lib):
    """The client's key upload as a seeded blob, N = 2^11: the keys expanded from the unpacked
    bundle (under unpacked seeded expansion keys) carry the round keys' bits, their worst deviation
    from +-1 at most 4 times that of the original bundle under the original keys."""
    e = Engine(_lib=oracle_lib, log_n=11, max_level=5, seed=41, special_primes=2, scale_bits=40)
    sk = e.create_secret_key(5)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), None)
    rks = T.expand_key(np.random.default_rng(2).integers(0, 256, 16, dtype=np.uint8))
    levels = [4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 3]
    bundle = R.encrypt_key_bundle(rks, level=5)
    blob = e.pack_ciphertext(bundle, sk, SEED)
    full = 128 + 2 * sum((q - 1).bit_length() for q in e.primes[:6]) * 2048 // 8
    assert len(blob) == 128 + (full - 128) // 2 < 2 * 6 * 2048 * 8 / 2.9
    xk = R.create_key_expansion_keys()
    xs = [e.unpack(e.pack_key(k, sk, SEED)) for k in xk]
    worst = []
    for b, keys in ((bundle, xk), (e.unpack(blob), xs)):
        out = R.expand_round_keys(b, keys, levels)
        w = 0.0
        for k in (0, 5, 10):
            for r in range(4):
                for j in range(8):
                    v = np.real(e.decrypt(out[k][r][j], sk))
                    want = np.array([1.0 - 2.0 * ((int(rks[k][r + 4 * c]) >> j) & 1) for c in range(4)])
                    w = max(w, float(np.abs(v - want[:, None]).max()))
        worst.append(w)
    print(f"expanded keys: worst deviation {worst[0]:.3e} original, {worst[1]:.3e} seeded")
    assert 0 < worst[1] <= 4 * worst[0] and worst[0] < 1e-3


# ------------------------------------------------------------------------------------------------
# 5. refusals, save / load
def _hdr(blob, **kw):
    """blob with header fields overwritten (offsets of wire_format.h)."""
    off = dict(magic=(0, "8s"), version=(8, "<I"), type=(12, "<I"), kind=(16, "<i"), ndig=(20, "<I"), galois=(24, "<Q"),
               batch=(40, "<i"),
               npoly=(44, "<i"), level=(48, "<i"), log_n=(52, "<i"), L=(56, "<i"), K=(60, "<i"), digest=(64, "<Q"),
               seeded=(72, "<I"), payload=(112, "<Q"))
    b = bytearray(blob)
    for name, v in kw.items():
        struct.pack_into(off[name][1], b, off[name][0], v)
    return bytes(b)


def _refusals(o):
    """(what, call, error text) of every refusal of the pack / unpack calls."""
    e, sk, pk = o["e"], o["sk"], o["pk"]
    gk = o["keys"]["galois"][0]
    kblob, cblob = e.pack_key(gk), e.pack_ciphertext(o["ct2"])
    L = e.max_level
    arg, deg = "invalid argument", "degree error"
    out = [
        ("seeded secret key", lambda: e.pack_key(sk, sk, SEED), arg),
        ("target not a secret key", lambda: e.pack_key(gk, pk, SEED), arg),
        ("ct sk not a secret key", lambda: e.pack_ciphertext(o["ct2"], pk, SEED), arg),
        ("seeded npoly 3", lambda: e.pack_ciphertext(o["ct3"], sk, SEED), deg),
        ("bad magic", lambda: e.unpack(_hdr(kblob, magic=b"AESFHEX\x00")), arg),
        ("bad version", lambda: e.unpack(_hdr(kblob, version=2)), arg),
        ("truncated", lambda: e.unpack(kblob[:-8]), arg),
        ("trailing bytes", lambda: e.unpack(cblob + bytes(8)), arg),
        ("short of a header", lambda: e.unpack(cblob[:100]), arg),
        ("payload field", lambda: e.unpack(_hdr(cblob, payload=len(cblob) - 128 - 8)), arg),
        ("chain digest", lambda: e.unpack(_hdr(kblob, digest=1)), arg),
        ("log_n", lambda: e.unpack(_hdr(kblob, log_n=e.log_coeff_count + 1)), arg),
        ("L", lambda: e.unpack(_hdr(cblob, L=L + 1)), arg),
        ("K", lambda: e.unpack(_hdr(cblob, K=3)), arg),
        ("digits above dnum", lambda: e.unpack(_hdr(kblob, ndig=e.dnum + 1)), arg),
        ("zero digits", lambda: e.unpack(_hdr(kblob, ndig=0)), arg),
        ("level above L", lambda: e.unpack(_hdr(cblob, level=L + 1)), arg),
        ("negative level", lambda: e.unpack(_hdr(cblob, level=-1)), arg),
        ("npoly 4", lambda: e.unpack(_hdr(cblob, npoly=4)), arg),
        ("batch 0", lambda: e.unpack(_hdr(cblob, batch=0)), arg),
        ("batch overflow", lambda: e.unpack(_hdr(cblob, batch=2 ** 31 - 1)), arg),
        ("unknown kind", lambda: e.unpack(_hdr(kblob, kind=4)), arg),
        ("unknown type", lambda: e.unpack(_hdr(kblob, type=3)), arg),
        ("seeded secret blob", lambda: e.unpack(_hdr(e.pack_key(sk), seeded=1)), arg),
        # the galois element is validated too: odd and below 2N for kinds 3 and 5, none otherwise
        ("galois element 2N + 1", lambda: e.unpack(_hdr(kblob, galois=(2 << e.log_coeff_count) + 1)), arg),
        ("galois element 2^64 - 3", lambda: e.unpack(_hdr(kblob, galois=2 ** 64 - 3)), arg),
        ("even galois element", lambda: e.unpack(_hdr(kblob, galois=6)), arg),
        ("galois element 0 in a galois key", lambda: e.unpack(_hdr(kblob, galois=0)), arg),
        ("galois element in a relinearisation key", lambda: e.unpack(_hdr(e.pack_key(o["keys"]["relin"][0]), galois=5)), arg),
        ("galois element in a public key", lambda: e.unpack(_hdr(e.pack_key(pk), galois=1)), arg),
        ("galois element in a ciphertext", lambda: e.unpack(_hdr(cblob, galois=1)), arg),
    ]
    # another engine's blob: another chain
    other = _objs(o["lib"], e.log_coeff_count, "A3" if o["chain"] == "A2" else "A2")
    out.append(("another chain", lambda: e.unpack(other["e"].pack_ciphertext(other["ct2"])), arg))
    return out


def _refuse_all(o):
    for what, call, text in _refusals(o):
        with pytest.raises(RuntimeError, match=text):
            call()
            pytest.fail(f"{what} was not refused")


def _zero_round_trip(o):
    e = o["e"]
    # a seed without the secret key would silently give the larger, unseeded blob
    for call in (lambda: e.pack_key(o["pk"], None, SEED), lambda: e.pack_ciphertext(o["ct2"], seed=SEED)):
        with pytest.raises(ValueError, match="seed without the secret key"):
            call()
    # any other odd element below 2N is accepted, and the class / rotation recovery ends
    gk = o["keys"]["galois"][0]
    for g, cls in ((3, GaloisKey), ((2 << e.log_coeff_count) - 3, FixedRotationKey), (1, GaloisKey)):
        k = e.unpack(_hdr(e.pack_key(gk), galois=g))
        assert type(k) is cls and k.galois_elt == g
        assert cls is GaloisKey or e._lib.galois_elt(e.log_coeff_count, k.delta, 0) == g
    assert e.unpack(e.pack_key(gk), delta=1 + e.slot_count).delta == 1 + e.slot_count  # a known rotation is taken as given
    zc = e.zeros(3, 2)
    for blob in (e.pack_ciphertext(zc), e.pack_ciphertext(zc, o["sk"], SEED)):
        assert len(blob) == 128
        c = e.unpack(blob)
        assert (c.batch, c.npoly, c.level, c.is_zero) == (3, 2, 2, True) and not e.export_residues(c).any()


@pytest.mark.parametrize("chain", ["A2", "A3"])
def test_refusals_oracle(oracle_lib, chain):
    o = dict(_objs(oracle_lib, 10, chain), lib=oracle_lib, chain=chain)
    _refuse_all(o)
    _zero_round_trip(o)


def test_save_compact_and_load_every_key_class(oracle_lib, tmp_path):
    o = _objs(oracle_lib, 10, "A2")
    e, sk = o["e"], o["sk"]
    objs = dict({n: k for n, k in o["keys"].items()}, secret=(sk, None))
    for name, (k, target) in objs.items():
        for seeded in ((False, True) if target is not None else (False,)):
            p = tmp_path / f"{name}{int(seeded)}.bin"
            e.save(k, p, compact=True, sk=target if seeded else None, seed=SEED if seeded else None)
            assert p.read_bytes() == e.pack_key(k, target if seeded else None, SEED if seeded else None)
            k2 = e.load(p)
            assert isinstance(k2, {SecretKey: SecretKey, PublicKey: PublicKey, RelinearizationKey: RelinearizationKey,
                                   ConjugationKey: ConjugationKey, FixedRotationKey: FixedRotationKey,
                                   GaloisKey: GaloisKey}[type(k)]), (name, type(k2))
            kind, g, ks, data = _export(e, k)
            kind2, g2, ks2, data2 = _export(e, k2)
            assert (kind2, g2, ks2, data2.size) == (kind, g, ks, data.size)
            assert np.array_equal(data2, data) == (not seeded)
        e.save(k, tmp_path / "full.bin")  # the existing format is untouched and still loads
        assert np.array_equal(_export(e, e.load(tmp_path / "full.bin"))[3], _export(e, k)[3])
        assert (tmp_path / "full.bin").stat().st_size > 1.2 * (tmp_path / f"{name}0.bin").stat().st_size
    for c, kw in ((o["ct2"], {}), (o["ct2"], dict(sk=sk, seed=SEED)), (o["ct3"], {})):
        e.save(c, tmp_path / "ct.bin", compact=True, **kw)
        c2 = e.load(tmp_path / "ct.bin")
        assert (c2.batch, c2.npoly, c2.level) == (c.batch, c.npoly, c.level)
        np.testing.assert_allclose(e.decrypt(c2, sk) if c.npoly == 2 else 0, e.decrypt(c, sk) if c.npoly == 2 else 0, atol=1e-4)
    with pytest.raises(TypeError):
        e.save(object(), tmp_path / "x.bin", compact=True)


def test_save_evaluation_keys_round_trip(oracle_lib, tmp_path):
    """A bootstrapper pair's keys (shared and trimmed ones included) and an AESSlicedRound's through
    save_evaluation_keys and its loader: every loaded key satisfies its seeded blob's structure --
    kind, galois element, stored digits -- and the two sparse switching keys (equal kind and galois
    element) got different masks."""
    from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys
    e = Engine(_lib=oracle_lib, log_n=10, max_level=14, seed=3, special_primes=4, scale_bits=40)
    sk = e.create_secret_key(1)
    rlk = e.create_relinearization_key(sk)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), rlk, e.create_conjugation_key(sk))
    bs = [Bootstrapper(e, sk, rlk, cts_groups=3)]
    bs.append(Bootstrapper(e, sk, rlk, cts_groups=5, share=bs[0]))
    trim_bootstrap_keys(bs)
    before = {n: (k, _export(e, k)) for n, (k, _) in
              ((n, v) for n, v in wire.evaluation_key_set(bs, R, None).items() if not isinstance(v, str))}
    info = wire.save_evaluation_keys(tmp_path, sk, SEED, bootstrappers=bs, rounds=R)
    files = sorted(p.name for p in tmp_path.glob("*.key"))
    assert len(files) == len(before) and info["bytes"] == sum((tmp_path / f).stat().st_size for f in files)
    assert info["bytes"] < info["full_bytes"] / 2.4  # seeded halves it, 50- and 40-bit rows in 64-bit words
    keys = wire.load_evaluation_keys(tmp_path, e, bootstrappers=bs, rounds=R)
    assert bs[0].to_sparse is keys["bs0.to_sparse"] and bs[1].from_sparse is bs[0].from_sparse and R.rlk is keys["rlk"]
    n = 1 << 10
    for name, (k, (kind, g, ks, data)) in before.items():
        kind2, g2, ks2, data2 = _export(e, keys[name])
        assert (kind2, g2, ks2, data2.size) == (kind, g, ks, data.size), name
        assert type(keys[name]) is type(k) and getattr(keys[name], "delta", None) == getattr(k, "delta", None)
    to_a = _rows_of(e, 3, _export(e, keys["bs0.to_sparse"])[3])[0, 1, 0]
    from_a = _rows_of(e, 3, _export(e, keys["bs0.from_sparse"])[3])[0, 1, 0]
    assert (to_a != from_a).sum() > n - 8
    # the identity for the key whose target is the ephemeral sparse secret
    s = _export(e, e.create_sparse_secret_key(*bs[0]._sparse_id))[3].reshape(-1, n).astype(object)
    orig = _rows_of(e, 3, before["bs0.to_sparse"][1][3])
    got = _rows_of(e, 3, _export(e, keys["bs0.to_sparse"])[3])
    _check_identity(e, orig, got[:, 0].astype(object), got[:, 1].astype(object), s)


# ------------------------------------------------------------------------------------------------
# 6. the sanitizer program
def test_wire_format_asan(tmp_path):
    """aes-fhe_amd/csrc/ext/wire_format.h under ASan + UBSan (tests/native/wire_format_asan.cpp): the
    parser and the host row codec over valid blobs, every truncation length of a small blob and
    headers with each count field at 0, its maximum and an overflowing product."""
    exe = tmp_path / "wire_format_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "wire_format_asan.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = tmp_path / "vec.bin"
    r = subprocess.run([str(exe), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wire_format_asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    # the host codec's vector against this file's integer packer and the package's numpy one:
    # 1024 residues of a 50-bit and of a 33-bit prime, the program's own xorshift values
    raw = out.read_bytes()
    off = 0
    for q in (1125899906826241, 8589148161):
        w = (q - 1).bit_length()
        res = np.frombuffer(raw, dtype="<u8", count=1024, offset=off)
        off += 8192
        packed = raw[off:off + 128 * w]
        off += 128 * w
        assert int(res.max()) < q
        assert packed == _pack_rows_int([(0, res)], [q]) == wire.pack_row(res, w)
        assert np.array_equal(wire.unpack_row(packed, 1024, w), res)
    assert off == len(raw)


# ------------------------------------------------------------------------------------------------
# GPU
def _parity(product_lib, oracle_lib, log_n, chain):
    g, o = _objs(product_lib, log_n, chain), _objs(oracle_lib, log_n, chain)
    ge, oe = g["e"], o["e"]
    assert ge._lib.has_ext and not oe._lib.has_ext
    for name in list(o["keys"]) + ["secret"]:
        (gk, gt), (ok, ot) = (g["keys"].get(name, (g["sk"], None)), o["keys"].get(name, (o["sk"], None)))
        for seeded in ((False, True) if ot is not None else (False,)):
            want = oe.pack_key(ok, ot if seeded else None, SEED if seeded else None)
            got = ge.pack_key(gk, gt if seeded else None, SEED if seeded else None)
            assert got == want, (name, seeded)
            # the fallback's blob unpacked on the device: the fallback's residues
            assert np.array_equal(_export(ge, ge.unpack(want))[3], wire.unpack_rows(oe, want)[1].reshape(-1)), (name, seeded)
    for name, seeded in (("ct2", False), ("ct2", True), ("ct3", False)):
        want = oe.pack_ciphertext(o[name], o["sk"] if seeded else None, SEED if seeded else None)
        assert ge.pack_ciphertext(g[name], g["sk"] if seeded else None, SEED if seeded else None) == want, (name, seeded)
        assert np.array_equal(ge.export_residues(ge.unpack(want)), wire.unpack_rows(oe, want)[1]), (name, seeded)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["A2", "A3"])
def test_blob_parity_gpu(product_lib, oracle_lib, gpu_available, chain):
    """N = 2^11, every key kind and both ciphertext shapes: the HIP engine's blobs are the
    fallback's byte for byte, and its unpack of them gives the fallback's residues."""
    _parity(product_lib, oracle_lib, 11, chain)


@pytest.mark.gpu
def test_blob_parity_full_shape_gpu(product_lib, oracle_lib, gpu_available):
    """N = 2^16, L = 30, K = 10, alpha = 12 (the ten-round shape): one galois key (3 digits, the
    last one short) and one batch-3 ciphertext."""
    kw = dict(log_n=16, max_level=30, special_primes=10, digit_primes=12, scale_bits=40, seed=5)
    blobs = []
    for lib in (product_lib, oracle_lib):
        e = Engine(_lib=lib, **kw)
        sk = e.create_secret_key(2)
        gk = e.create_fixed_rotation_key(sk, 5)
        e._nonce = 40
        ct = e.encrypt(np.exp(2j * np.pi * np.random.default_rng(8).integers(0, 16, (3, e.slot_count)) / 16),
                       e.create_public_key(sk), level=7)
        blobs.append((e, e.pack_key(gk, sk, SEED), e.pack_ciphertext(ct, sk, SEED), e.pack_ciphertext(ct), gk, ct))
    (g, gkb, gcs, gcu, gk, ct), (o, okb, ocs, ocu, _, _) = blobs
    assert g.dnum == 3 and len(okb) == _size(o, 3, 1, 41)
    assert gkb == okb and gcs == ocs and gcu == ocu
    assert np.array_equal(_export(g, g.unpack(okb))[3], wire.unpack_rows(o, okb)[1].reshape(-1))
    assert np.array_equal(g.export_residues(g.unpack(ocs)), wire.unpack_rows(o, ocs)[1])
    assert np.array_equal(g.export_residues(g.unpack(ocu)), g.export_residues(ct))
    del blobs, gk, ct
    gc.collect()
    g.pool_trim()


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


@pytest.mark.gpu
def test_refusals_and_launch_count_gpu(product_lib, gpu_available):
    o = dict(_objs(product_lib, 11, "A2"), lib=product_lib, chain="A2")
    _objs(product_lib, 11, "A3")  # the other chain's engine exists before the baseline
    e = o["e"]
    gk = o["keys"]["hoisted"][0]
    blob, prof = _profiled(e, lambda: e.pack_key(gk, o["sk"], SEED))
    # per class: calls, milliseconds, bytes, kernel dispatches
    assert set(prof) == {"wire_pack"} and (prof["wire_pack"][0], prof["wire_pack"][3]) == (1, 1), prof
    k2, prof = _profiled(e, lambda: e.unpack(blob))
    assert set(prof) == {"wire_unpack"} and (prof["wire_unpack"][0], prof["wire_unpack"][3]) == (1, 1), prof
    _, prof = _profiled(e, lambda: e.unpack(e.pack_ciphertext(o["ct3"])))
    assert set(prof) == {"wire_pack", "wire_unpack"} and all((v[0], v[3]) == (1, 1) for v in prof.values()), prof
    del k2
    # a residue forced to q
    res = e.export_residues(o["ct2"])
    res[1, 1, 2, 1029] = e.primes[2]
    order = [(l, res[b, p, l]) for b in range(3) for p in range(2) for l in range(res.shape[2])]
    forced = e.pack_ciphertext(o["ct2"])[:128] + _pack_rows_int(order, e.primes)
    gc.collect()
    e.synchronize()
    base = e.pool_stats()["live"]
    _refuse_all(o)
    with pytest.raises(RuntimeError, match="invalid argument.*not below its prime"):
        e.unpack(forced)
    gc.collect()
    e.synchronize()
    assert e.pool_stats()["live"] == base
    _zero_round_trip(o)
    assert np.array_equal(e.export_residues(e.unpack(e.pack_ciphertext(o["ct2"]))), e.export_residues(o["ct2"]))


@pytest.mark.gpu
def test_product_path_under_loaded_keys_gpu(product_lib, gpu_available, tmp_path):
    """N = 2^12, tests/test_ctr.py's reduced pipeline (ARK0 by counter planes, one middle round, the
    final round under the data-folded key): the server's engine holds only what came through
    save_evaluation_keys' files and a seeded bundle blob, and the state decrypts to the message."""
    nb = 2
    rng = np.random.default_rng(3)
    rks = T.expand_key(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + bytes.fromhex("fffffe00")
    first = 100
    e = Engine(_lib=product_lib, log_n=12, max_level=14, seed=21, special_primes=4, scale_bits=40)
    sk = e.create_secret_key(5)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
    L = e.max_level - 1
    data = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    l1, lk = L - 1 - R.KEY_OFFSET, L - 1 - 7 - R.KEY_OFFSET
    levels = [L, l1] + [0] * 8 + [lk + 1]
    # the client: evaluation keys and the bundle, as files
    info = wire.save_evaluation_keys(tmp_path, sk, SEED, rounds=R, expansion_keys=R.create_key_expansion_keys())
    e.save(R.encrypt_key_bundle(rks, level=L + 1), tmp_path / "bundle.ct", compact=True, sk=sk, seed=SEED2)
    assert info["bytes"] < info["full_bytes"] / 2.4
    # the server: the same engine parameters, nothing but the files
    S = AESSlicedRound(e, sk, R.pk, None)
    keys = wire.load_evaluation_keys(tmp_path, e, rounds=S)
    assert S.rlk is keys["rlk"] is not R.rlk and len(keys["expansion"]) == 11
    rk = S.expand_round_keys(e.load(tmp_path / "bundle.ct"), keys["expansion"], levels)
    st = S.counter_state(rk[0], iv, nb, first)
    st = S.round(st, rk[1])
    st = S.final_round(st, S.fold_data_key(rk[10], data))
    ctr = T.ctr_blocks(iv, nb * S.n_blk, first).reshape(nb, S.n_blk, 16)
    want = T.shift_rows(T.sub_bytes(T.aes_round(ctr ^ rks[0], rks[1]))) ^ rks[10] ^ data
    assert np.array_equal(S.decrypt_blocks(st, nb), want)

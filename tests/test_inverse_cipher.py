"""AES-128 decryption (aes_round_bits.AESSlicedDecrypt): the equivalent
inverse cipher in T-table form -- one 32-output S-box call per row, a five-leaf product per
output bit -- and ECB / CBC transciphering on it.

CPU: the plain models against FIPS-197 C.1 and NIST SP 800-38A F.1 / F.2, the Walsh weights of
the inverse S-box and of its four InvMixColumns multiples, one round and the final round on the
oracle (two slabs, the second half padding), a whole CBC transciphering on the oracle at N = 2^10
with the bench's ten-round settings, a reduced ECB one, the refusals.  GPU: a reduced CBC pipeline
and the 32-output S-box call at N = 2^16, both residue-exact against the oracle, and one slab of
transcipher_cbc at N = 2^16, L = 30."""
from types import SimpleNamespace

import numpy as np
import pytest

from aes_xor_fhe import aes_tables as T
from aes_xor_fhe.aes_round_bits import INV_MIX, AESSlicedDecrypt, AESSlicedRound, walsh_inv_sbox, walsh_inv_tbox
from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys
from aes_xor_fhe.fhe import Engine
from test_aes128_full import BENCH10
from _ks_helpers import _compare, _drop, _pair, _pool

FIPS_KEY = bytes(range(16))
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS_CT = bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")
NIST_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
NIST_IV = bytes(range(16))
NIST_PT = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51")
NIST_ECB = bytes.fromhex("3ad77bb40d7a3660a89ecaf32466ef97" "f5d3d58503b9699de785895a96fdbaaf")
NIST_CBC = bytes.fromhex("7649abac8119b246cee98e9b12e9197d" "5086cb9b507219ee95db113a917678b2")


def _b(x, n=1):
    return np.frombuffer(x, np.uint8).reshape(n, 16)


# ------------------------------------------------------------------------------------------------
# 1. the plain models
def test_decrypt_block_fips197_c1():
    assert np.array_equal(T.encrypt_block(_b(FIPS_PT)[0], FIPS_KEY), _b(FIPS_CT)[0])  # the vector as typed
    assert np.array_equal(T.decrypt_block(_b(FIPS_CT)[0], FIPS_KEY), _b(FIPS_PT)[0])
    dk = T.decryption_keys(FIPS_KEY)
    rk = T.expand_key(FIPS_KEY)
    assert dk.shape == (11, 16) and dk.dtype == np.uint8
    assert np.array_equal(dk[0], rk[10]) and np.array_equal(dk[10], rk[0])
    assert all(np.array_equal(dk[i], T.inv_mix_columns(rk[10 - i])) for i in range(1, 10))
    assert np.array_equal(T.eq_decrypt_block(_b(FIPS_CT)[0], dk), _b(FIPS_PT)[0])


def test_nist_sp800_38a_ecb_and_cbc_aes128():
    pt, ecb, cbc, iv = _b(NIST_PT, 2), _b(NIST_ECB, 2), _b(NIST_CBC, 2), _b(NIST_IV)[0]
    # the typed vectors against the FIPS-197-pinned block cipher first
    assert np.array_equal(T.encrypt_block(pt, NIST_KEY), ecb)
    assert np.array_equal(T.encrypt_block(pt[0] ^ iv, NIST_KEY), cbc[0])
    assert np.array_equal(T.encrypt_block(pt[1] ^ cbc[0], NIST_KEY), cbc[1])
    assert np.array_equal(T.ecb_encrypt(pt, NIST_KEY), ecb) and np.array_equal(T.ecb_decrypt(ecb, NIST_KEY), pt)
    assert np.array_equal(T.cbc_encrypt(pt, NIST_KEY, NIST_IV), cbc)
    assert np.array_equal(T.cbc_decrypt(cbc, NIST_KEY, NIST_IV), pt)
    # a later chunk takes the block before its first as its chaining value
    assert np.array_equal(T.cbc_decrypt(cbc[1:], NIST_KEY, cbc[0]), pt[1:])
    with pytest.raises(ValueError, match="16 bytes"):
        T.cbc_decrypt(cbc, NIST_KEY, bytes(15))


def test_equivalent_inverse_cipher_and_cbc_round_trip_on_random_blocks():
    rng = np.random.default_rng(0)
    key, iv = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, 16, dtype=np.uint8)
    x = rng.integers(0, 256, (3, 5, 16), dtype=np.uint8)
    dk = T.decryption_keys(key)
    assert np.array_equal(T.eq_decrypt_block(x, dk), T.decrypt_block(x, key))
    assert np.array_equal(T.decrypt_block(T.encrypt_block(x, key), key), x)
    # one middle round of the equivalent cipher is the straight one's with the key moved through
    # InvMixColumns (which is linear)
    rk = T.expand_key(key)
    assert np.array_equal(T.eq_inv_round(x, dk[1]),
                          T.inv_mix_columns(T.inv_shift_rows(T.INV_SBOX[x]) ^ rk[9]))
    enc = T.cbc_encrypt(x, key, iv)
    assert enc.shape == x.shape and not np.array_equal(enc, x)
    assert np.array_equal(T.cbc_decrypt(enc, key, iv), x)
    assert np.array_equal(T.ecb_decrypt(T.ecb_encrypt(x, key), key), x)
    # blocks are counted in C order: the second set chains on the last block of the first
    assert np.array_equal(T.cbc_decrypt(enc[1], key, enc[0, -1]), x[1])
    assert np.array_equal(T.cbc_previous(enc, iv).reshape(-1, 16)[1:], enc.reshape(-1, 16)[:-1])


# ------------------------------------------------------------------------------------------------
# 2. the weights
def _monomial_values():
    """mono[mask, nibble]: the +-1 product of the nibble's bits in `mask`."""
    return np.array([[np.prod([1 - 2 * ((v >> k) & 1) for k in range(4) if (m >> k) & 1]) for v in range(16)]
                     for m in range(16)], dtype=np.float64)


def test_walsh_weights_reproduce_every_bit_of_every_multiple():
    Wt, Wi = walsh_inv_tbox(), walsh_inv_sbox()
    assert Wt.shape == (4, 8, 16, 16) and Wi.shape == (8, 16, 16)
    assert INV_MIX == (0x0E, 0x0B, 0x0D, 0x09)
    mono = _monomial_values()
    x = np.arange(256)
    mh, ml = mono[:, x >> 4], mono[:, x & 15]  # [mask, byte]
    inv = T.INV_SBOX[x].astype(np.int64)
    tables = [inv] + [np.array([T.gf_mul(int(v), c) for v in inv]) for c in INV_MIX]
    for W, tab in zip([Wi] + list(Wt), tables):
        got = np.einsum("tsu,sx,ux->tx", W, mh, ml)  # the monomial sums, all 256 bytes
        want = np.stack([1.0 - 2.0 * ((tab >> t) & 1) for t in range(8)])
        assert np.array_equal(got, want)
    for W in (Wt, Wi):
        W64 = W * 64
        assert np.array_equal(W64, np.rint(W64)) and W64.min() >= -8 and W64.max() <= 8
        assert np.abs(W64).sum(axis=-1).max() <= 512  # poly2_int's bound on a row of weights
    assert np.array_equal(Wt[0], walsh_inv_tbox()[0]) and not np.array_equal(Wt[0], Wt[1])


# ------------------------------------------------------------------------------------------------
# 3. one round and the final round on the oracle: two slabs, the second half padding
@pytest.fixture(scope="module")
def one_round(oracle_lib):
    e = Engine(log_n=10, max_level=13, seed=21, _lib=oracle_lib, special_primes=8)
    sk = e.create_secret_key(3)
    R = AESSlicedDecrypt(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
    nb = 6
    rng = np.random.default_rng(5)
    dk = T.decryption_keys(rng.integers(0, 256, 16, dtype=np.uint8))
    blocks = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    S = R.encrypt_blocks(blocks)
    L = e.max_level
    assert all(c.level == L and c.batch == 8 for row in S for c in row)
    calls, key_muls = [], []
    p2, key_mul = e.poly2_int, R.key_mul

    def poly2_int(xb, yb, W, den, rlk, slab_rot=0):
        calls.append((np.asarray(W).shape, den, slab_rot))
        return p2(xb, yb, W, den, rlk, slab_rot=slab_rot)
    e.poly2_int = poly2_int
    R.key_mul = lambda a, k: (key_muls.append((a.level, k.level, a.batch, k.batch)), key_mul(a, k))[1]
    try:
        tm = {}
        A = R.round(S, R.encrypt_round_key(dk[1], level=L - R.KEY_OFFSET), tm)
        n_round = len(calls)
        F = R.final_round(A, R.encrypt_round_key(dk[10], level=A[0][0].level - R.KEY_OFFSET))
    finally:
        del e.poly2_int, R.key_mul
    return SimpleNamespace(e=e, R=R, nb=nb, dk=dk, blocks=blocks, L=L, A=A, F=F, calls=calls, n_round=n_round,
                           key_muls=key_muls, tm=tm)


def test_round_is_the_equivalent_inverse_round_in_seven_levels(one_round):
    t = one_round
    assert t.R.ROUND_DEPTH == 7 and t.R.FINAL_DEPTH == 5 and t.R.KEY_OFFSET == 4
    assert all(c.level == t.L - 7 and c.batch == 8 for row in t.A for c in row)
    assert np.array_equal(t.R.decrypt_blocks(t.A, t.nb), T.eq_inv_round(t.blocks, t.dk[1]))
    assert set(t.tm) == {"inv_sub_bytes_shift_rows_mix", "inv_mix_columns_add_round_key"}
    # the key met the S-box outputs at their level, cycled (batch 4 against two slabs)
    assert t.key_muls[:32] == [(t.L - 4, t.L - 4, 8, 4)] * 32


def test_final_round_in_five_levels(one_round):
    t = one_round
    assert all(c.level == t.L - 7 - 5 and c.batch == 8 for row in t.F for c in row)
    mid = T.eq_inv_round(t.blocks, t.dk[1])
    assert np.array_equal(t.R.decrypt_blocks(t.F, t.nb), T.inv_shift_rows(T.INV_SBOX[mid]) ^ t.dk[10])
    assert t.key_muls[32:] == [(t.L - 7 - 4, t.L - 7 - 4, 8, 4)] * 32
    assert t.R.bit_margin(t.F) < 1e-3


def test_sbox_step_is_one_call_of_32_outputs_per_row(one_round):
    t = one_round
    assert t.n_round == 4
    assert t.calls[:4] == [((32, 16, 16), 64, (4 - r) % 4) for r in range(4)]
    assert t.calls[4:] == [((8, 16, 16), 64, (4 - r) % 4) for r in range(4)]


def test_previous_blocks_numpy_and_torch_agree():
    """The shifted ciphertext as the HIP engine builds it (torch) is the oracle's (numpy)."""
    import torch
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, (6, 16, 16), dtype=np.uint8)
    iv = rng.integers(0, 256, 16, dtype=np.uint8)
    R = AESSlicedDecrypt.__new__(AESSlicedDecrypt)
    R.sc, R.n_blk = 64, 16
    R.e = SimpleNamespace(on_device=False)
    a = R.previous_blocks(data, bytes(iv))
    R.e = SimpleNamespace(on_device=True, client_device=torch.device("cpu"))
    b = R.previous_blocks(torch.from_numpy(data), iv)
    assert np.array_equal(a, b.numpy()) and np.array_equal(a, T.cbc_previous(data, iv))
    assert np.array_equal(a[0, 0], iv) and np.array_equal(a[3, 0], data[2, 15])


# ------------------------------------------------------------------------------------------------
# 4. whole transcipherings on the oracle
def _setup(lib, log_n, seed=3):
    kw = {k: v for k, v in BENCH10.items() if k not in ("cls", "cts_groups", "key_levels")}
    e = Engine(log_n=log_n, max_level=30, seed=seed, _lib=lib, **kw)
    sk = e.create_secret_key(1)
    rlk = e.create_relinearization_key(sk)
    assert BENCH10["cls"] is AESSlicedRound
    R = AESSlicedDecrypt(e, sk, e.create_public_key(sk), rlk)
    bs = []
    for g in BENCH10["cts_groups"]:
        bs.append(Bootstrapper(e, sk, rlk, cts_groups=g, share=bs[0] if bs else None))
    trim_bootstrap_keys(bs)
    return e, R, bs


def _transcipher_cbc(lib, log_n, nb, seed=3):
    """transcipher_cbc of nb sets encrypted with cbc_encrypt, every key product and every batched
    plaintext product recorded."""
    e, R, bs = _setup(lib, log_n, seed)
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    iv = rng.integers(0, 256, 16, dtype=np.uint8)
    msg = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    data = T.cbc_encrypt(msg, key, iv)
    L0 = R.fresh_level(e.max_level, bs)
    levels = R.ctr_key_levels(L0, bs)
    keys = [R.encrypt_round_key(k, level=v) for k, v in zip(T.decryption_keys(key), levels)]
    key_muls, plain_muls = [], []
    key_mul, mpb = R.key_mul, e.multiply_plain_batch
    R.key_mul = lambda a, k: (key_muls.append((a.level, k.level, a.batch, k.batch)), key_mul(a, k))[1]
    e.multiply_plain_batch = lambda ct, pb: (plain_muls.append((ct.level, ct.batch, pb.batch)), mpb(ct, pb))[1]
    tm = {}
    try:
        out, nref = R.transcipher_cbc(data, iv, keys, bs, timings=tm)
    finally:
        del R.key_mul, e.multiply_plain_batch
    return SimpleNamespace(e=e, R=R, bs=bs, L0=L0, levels=levels, out=out, nref=nref, tm=tm, msg=msg, data=data,
                           key=key, iv=iv, key_muls=key_muls, plain_muls=plain_muls, nb=nb)


def _check_transcipher_cbc(t):
    R, S4 = t.R, 4 * t.R.slabs(t.nb)
    assert t.nref == 3
    assert all(c.level == 0 and c.batch == S4 for row in t.out for c in row)
    # every round started at the level schedule() planned from L0 (state 0 at L0 - 1)
    sched = R.schedule(t.L0, t.bs)
    assert [lv for _, lv, _ in t.tm["per_round"]] == [lv for _, lv, _ in sched]
    assert t.L0 == 25 and sched[0][1] == t.L0 - 1 and sched[-1][1] == 5
    # the 64 batched plaintext products: the fold of the shifted ciphertext into dk_10 (one level
    # above the one round 10 consumes) first, then dk_0 times the data planes
    assert t.levels == R.key_levels(t.L0, t.bs)[:-1] + [R.key_levels(t.L0, t.bs)[-1] + 1]
    assert t.plain_muls == [(t.levels[10], 4, S4)] * 32 + [(t.L0, 4, S4)] * 32
    # every key product met its key at the state's level, the last under the folded key
    assert len(t.key_muls) == 32 * 10
    assert all(a == k for a, k, _, _ in t.key_muls)
    assert t.key_muls[-32:] == [(sched[-1][1] - R.KEY_OFFSET, t.levels[10] - 1, S4, S4)] * 32
    assert all(kb == 4 for _, _, _, kb in t.key_muls[:-32])
    assert np.array_equal(T.cbc_decrypt(t.data, t.key, t.iv), t.msg)  # the model, block for block
    assert np.array_equal(R.decrypt_blocks(t.out, t.nb), t.msg)


def test_transcipher_cbc_ten_rounds_oracle(oracle_lib):
    _check_transcipher_cbc(_transcipher_cbc(oracle_lib, 10, nb=2))


def test_transcipher_ecb_reduced_oracle(oracle_lib, monkeypatch):
    """transcipher_ecb's own code -- the checks, state 0 from the data planes, the hand-over to
    cipher_rounds with the keys at key_levels -- on a cipher reduced to rounds 1 and 10 (the
    whole ten rounds run in the CBC test above, through the same cipher_rounds)."""
    e = Engine(log_n=10, max_level=13, seed=4, _lib=oracle_lib, special_primes=8)
    sk = e.create_secret_key(3)
    R = AESSlicedDecrypt(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
    rng = np.random.default_rng(8)
    dk = T.decryption_keys(rng.integers(0, 256, 16, dtype=np.uint8))
    nb = 2
    data = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    bs = [SimpleNamespace(bits_level=17, stc_bits=[0] * 3)]
    L = e.max_level
    seen = {}

    def two_rounds(S, keys, bss, **kw):
        seen["levels"] = {c.level for row in S for c in row}
        seen["kw"] = kw
        return R.final_round(R.round(S, keys[1]), keys[10]), 0
    monkeypatch.setattr(R, "cipher_rounds", two_rounds)
    levels = [L, L - 1 - 4] + [0] * 8 + [L - 1 - 7 - 4]
    monkeypatch.setattr(R, "key_levels", lambda *a, **k: levels)
    keys = [R.encrypt_round_key(k, level=v) for k, v in zip(dk, levels)]
    out, nref = R.transcipher_ecb(data, keys, bs)
    assert seen["levels"] == {L - 1} and seen["kw"] == {"out_level": 0} and nref == 0
    assert all(c.level == 0 and c.batch == 4 for row in out for c in row)
    want = T.inv_shift_rows(T.INV_SBOX[T.eq_inv_round(data ^ dk[0], dk[1])]) ^ dk[10]
    assert np.array_equal(R.decrypt_blocks(out, nb), want)


# ------------------------------------------------------------------------------------------------
# 5. the refusals: stub keys, nothing encrypted
def test_refusals_before_any_ciphertext_work(oracle_lib):
    e = Engine(log_n=10, max_level=30, seed=1, _lib=oracle_lib, special_primes=4, scale_bits=40)
    sk = e.create_secret_key(1)
    R = AESSlicedDecrypt(e, sk, e.create_public_key(sk), None)
    bs = [SimpleNamespace(bits_level=17, stc_bits=[0] * 3), SimpleNamespace(bits_level=19, stc_bits=[0] * 3)]
    touched = []
    e.multiply_plain_batch = lambda *a: touched.append(a)
    e.encode_batch = lambda *a: touched.append(a)
    good = np.zeros((2, R.n_blk, 16), np.uint8)
    ecb = [[[SimpleNamespace(level=v)]] for v in R.key_levels(25, bs)]
    cbc = [[[SimpleNamespace(level=v)]] for v in R.ctr_key_levels(25, bs)]
    for bad in (np.zeros((2, R.n_blk + 1, 16), np.uint8), np.zeros((R.n_blk, 16), np.uint8),
                np.zeros((2, R.n_blk, 15), np.uint8)):
        with pytest.raises(ValueError, match="data must be"):
            R.transcipher_ecb(bad, ecb, bs)
        with pytest.raises(ValueError, match="data must be"):
            R.transcipher_cbc(bad, bytes(16), cbc, bs)
    for iv in (bytes(15), bytes(17), np.zeros((1, 16), np.uint8)):
        with pytest.raises(ValueError, match="iv must be"):
            R.transcipher_cbc(good, iv, cbc, bs)
    # each method wants its own levels: CBC folds into the last key one level up
    with pytest.raises(ValueError, match="ctr_key_levels"):
        R.transcipher_cbc(good, bytes(16), ecb, bs)
    with pytest.raises(ValueError, match="key_levels"):
        R.transcipher_ecb(good, cbc, bs)
    with pytest.raises(ValueError, match="11 decryption keys"):
        R.transcipher_ecb(good, ecb[:10], bs)
    # keys for out_level 0 do not sit where a tail of 2 levels needs them
    with pytest.raises(ValueError, match="out_level=2"):
        R.transcipher_cbc(good, bytes(16), cbc, bs, out_level=2)
    # an out_level no bootstrapper can leave: a refresh returns level 19 at most, round 10 spends 5
    with pytest.raises(ValueError, match="out_level 15"):
        R.transcipher_cbc(good, bytes(16), cbc, bs, out_level=15)
    with pytest.raises(ValueError, match="out_level 15"):
        R.transcipher_ecb(good, ecb, bs, out_level=15)
    assert not touched


# ------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, dict(special_primes=10, digit_primes=12, scale_bits=40)], ids=["K8", "K10A12"])
def test_cbc_reduced_pipeline_bit_exact_vs_oracle(product_lib, oracle_lib, gpu_available, kw):
    """dk_0 times the data planes -> one middle round -> the final round under the key with the
    shifted ciphertext folded in, at N = 2^12: all 32 outputs residue-equal to the oracle's, and
    they decrypt to the plain model of that pipeline.  Two slabs, the second half padding.  The
    chain holds the 1 + 7 + 5 levels the pipeline uses."""
    nb = 6
    rng = np.random.default_rng(3)
    dk = T.decryption_keys(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = rng.integers(0, 256, 16, dtype=np.uint8)
    data = rng.integers(0, 256, (nb, (1 << 11) // 4, 16), dtype=np.uint8)
    want = T.inv_shift_rows(T.INV_SBOX[T.eq_inv_round(data ^ dk[0], dk[1])]) ^ dk[10] ^ T.cbc_previous(data, iv)
    outs = []
    for lib in (product_lib, oracle_lib):
        e = Engine(log_n=12, max_level=13, seed=21, _lib=lib, **dict(dict(special_primes=8), **kw))
        sk = e.create_secret_key(3)
        R = AESSlicedDecrypt(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
        L = e.max_level
        S = R.mul_planes(R.encrypt_round_key(dk[0], level=L), R.data_planes(data))
        assert all(c.level == L - 1 and c.batch == 8 for row in S for c in row)
        S = R.round(S, R.encrypt_round_key(dk[1], level=L - 1 - R.KEY_OFFSET))
        lk = S[0][0].level - R.KEY_OFFSET  # the level the final round's key product consumes
        K = R.fold_data_key(R.encrypt_round_key(dk[10], level=lk + 1), R.previous_blocks(data, iv))
        assert all(c.level == lk and c.batch == 8 for row in K for c in row)
        S = R.final_round(S, K)
        assert all(c.level == lk - 1 == 0 for row in S for c in row)
        assert np.array_equal(R.decrypt_blocks(S, nb), want)
        outs.append((e, S))
    (g, sg), (o, so) = outs
    assert g._lib.backend == "hip-gfx950"
    for rg, ro in zip(sg, so):
        for cg, co in zip(rg, ro):
            assert np.array_equal(g.export_residues(cg), o.export_residues(co))


@pytest.mark.gpu
def test_sbox_call_of_32_outputs_bit_exact_at_full_ring(product_lib, oracle_lib, gpu_available):
    """One row's S-box call of the inverse round where the fused base conversion runs: N = 2^16,
    K = 10, alpha = 12, B = 4, the 32-output table, slab_rot = 3, on the shortest chain that holds
    it -- singles at level 4, pairs at 3, triples and the quadruple at 2 (monomials' levels), so
    the relinearisation runs at l = 2 with batch 128 and two rescales.  All 32 outputs
    residue-equal to the oracle's."""
    g, o = _pair(product_lib, oracle_lib, log_n=16, max_level=4, special_primes=10, digit_primes=12, scale_bits=40,
                 seed=77)
    try:
        assert g._lib.backend == "hip-gfx950"
        W = np.rint(walsh_inv_tbox() * 64).astype(np.int64).reshape(32, 16, 16)
        levels = [4 - (0, 0, 1, 2, 2)[bin(m).count("1")] for m in range(1, 16)]
        assert min(levels) == 2 and levels[0] == 4 and levels[2] == 3
        base = _pool(g.primes, 4, 4, 4, seed=2032)  # polys 0-1: x, 2-3: y; monomial i: rolled by i
        outs = []
        for eng in (g, o):
            rlk = eng.create_relinearization_key(eng.create_secret_key(9))
            xb = [eng.import_residues(np.roll(base[:, 0:2, :lv + 1], 17 * i, axis=-1)) for i, lv in enumerate(levels)]
            yb = [eng.import_residues(np.roll(base[:, 2:4, :lv + 1], 29 * i, axis=-1)) for i, lv in enumerate(levels)]
            outs.append(eng.poly2_int(xb, yb, W, 64, rlk, slab_rot=3))
            del xb, yb, rlk
        _compare(g, o, outs[0], outs[1], [(0, 4, False)] * 32,
                 "op poly2_int (32-output inverse T-box weights, slab_rot 3), level 2, batch 4")
        del outs
    finally:
        _drop(g, o)


@pytest.mark.gpu
def test_transcipher_cbc_full_params(product_lib, gpu_available):
    """N = 2^16, L = 30, the bench's ten-round settings, one slab (4 sets, 32 768 blocks).
    Measured on an MI355X: see DESIGN.md section 5.5."""
    t = _transcipher_cbc(product_lib, 16, nb=4)
    assert t.e._lib.backend == "hip-gfx950"
    _check_transcipher_cbc(t)
    margin = t.R.bit_margin(t.out)
    print(f"transcipher_cbc N=2^16 nb=4: bit_margin {margin:.4f}, rounds {t.tm['rounds']:.2f} s, "
          f"bootstrap {t.tm['bootstrap']:.2f} s")
    assert margin < 1.0

"""AES-128-CTR transciphering (aes_round_bits.AESSlicedRound.keystream_aes128 / transcipher;
DESIGN.md section 5): the counter blocks enter as per-element plaintexts (no encrypted input
state), the symmetric ciphertext is folded into the last round key.

CPU: the plain CTR model against NIST SP 800-38A F.5.1, and the whole transciphering on the
oracle at N = 2^10 with the bench's ten-round settings.  GPU: a reduced pipeline (ARK0 by counter
planes, one middle round, the final round under the folded key) residue-exact against the oracle
at N = 2^12, and the whole run at N = 2^16, L = 30."""
from types import SimpleNamespace

import numpy as np
import pytest

from aes_xor_fhe import aes_tables as T
from aes_xor_fhe.aes_round_bits import AESSlicedRound
from aes_xor_fhe.bootstrap import Bootstrapper, trim_bootstrap_keys
from aes_xor_fhe.fhe import Engine
from test_aes128_full import BENCH10

NIST_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
NIST_CTR = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
NIST_PT = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51")
NIST_CT = bytes.fromhex("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff")


# ------------------------------------------------------------------------------------------------
# the plain model
def test_nist_sp800_38a_ctr_aes128():
    pt, ct = np.frombuffer(NIST_PT, np.uint8).reshape(2, 16), np.frombuffer(NIST_CT, np.uint8).reshape(2, 16)
    # the typed vector against the FIPS-197-pinned block cipher first: block 1's keystream is
    # AES(counter), block 2's AES(counter + 1) with the carry into byte 14
    ctr1 = np.frombuffer(NIST_CTR, np.uint8)
    ctr2 = np.frombuffer(bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdff00"), np.uint8)
    assert np.array_equal(T.encrypt_block(ctr1, NIST_KEY) ^ pt[0], ct[0])
    assert np.array_equal(T.encrypt_block(ctr2, NIST_KEY) ^ pt[1], ct[1])
    assert np.array_equal(T.ctr_blocks(NIST_CTR, 2), np.stack([ctr1, ctr2]))
    assert np.array_equal(T.ctr_xor(pt, NIST_KEY, NIST_CTR), ct)
    assert np.array_equal(T.ctr_xor(ct[1:], NIST_KEY, NIST_CTR, first=1), pt[1:])


def test_ctr_xor_inverts_itself():
    rng = np.random.default_rng(0)
    key, iv = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, 16, dtype=np.uint8)
    msg = rng.integers(0, 256, (3, 5, 16), dtype=np.uint8)
    enc = T.ctr_xor(msg, key, iv, first=7)
    assert enc.shape == msg.shape and not np.array_equal(enc, msg)
    assert np.array_equal(T.ctr_xor(enc, key, iv, first=7), msg)
    # blocks are counted in C order: the second set continues the first
    assert np.array_equal(T.ctr_xor(msg[1], key, iv, first=7 + 5), enc[1])


def test_ctr_blocks_wrap_in_the_last_four_bytes_only():
    iv = bytes(range(100, 112)) + bytes.fromhex("fffffffe")
    b = T.ctr_blocks(iv, 4)
    assert [bytes(x[12:]).hex() for x in b] == ["fffffffe", "ffffffff", "00000000", "00000001"]
    assert all(bytes(x[:12]) == iv[:12] for x in b)  # no carry into byte 11
    assert np.array_equal(T.ctr_blocks(iv, 2, first=2), b[2:])
    assert np.array_equal(T.ctr_blocks(iv, 1, first=2 ** 32), b[:1])
    assert T.ctr_blocks(iv, 0).shape == (0, 16)


def test_counter_planes_layout_and_device_rows():
    """counter_planes in the sliced layout: element 4 s + c, slot k is byte r + 4c of counter
    block first + s * slot_count + k; the torch construction (the HIP engine's) gives the numpy one."""
    import torch
    R = AESSlicedRound.__new__(AESSlicedRound)
    R.sc, R.n_blk = 64, 16
    R.e = SimpleNamespace(on_device=False)
    iv = bytes(range(12)) + bytes.fromhex("ffffffc0")
    first, nb = 5, 6  # two slabs (the second half padding); the counter wraps at block 59
    planes = R.counter_planes(iv, nb, first)
    blocks = T.ctr_blocks(iv, 2 * 64, first)
    assert blocks[59, 12:].tolist() == [0, 0, 0, 0] and blocks[58, 12:].tolist() == [255] * 4
    for r, c, s, k, j in [(0, 0, 0, 0, 0), (3, 3, 0, 59, 7), (3, 3, 1, 17, 2), (2, 1, 1, 63, 5), (1, 2, 0, 58, 0)]:
        bit = (int(blocks[s * 64 + k, r + 4 * c]) >> j) & 1
        assert planes[r][j][4 * s + c, k] == 1.0 - 2.0 * bit
    assert all(p.shape == (8, 64) and set(np.unique(p)) <= {-1.0, 1.0} for row in planes for p in row)
    rows = R.counter_rows_device(iv, 2, first, torch.device("cpu"))
    want = R.pack(blocks.reshape(8, 16, 16))
    for a, b in zip(rows, want):
        assert np.array_equal(a.numpy(), b)
    tp = R._sign_planes(rows)
    assert all(np.array_equal(tp[r][j].numpy(), planes[r][j]) for r in range(4) for j in range(8))


# ------------------------------------------------------------------------------------------------
# the homomorphic run
def _setup(lib, log_n, seed=3):
    kw = {k: v for k, v in BENCH10.items() if k not in ("cls", "cts_groups", "key_levels")}
    e = Engine(log_n=log_n, max_level=30, seed=seed, _lib=lib, **kw)
    sk = e.create_secret_key(1)
    rlk = e.create_relinearization_key(sk)
    R = BENCH10["cls"](e, sk, e.create_public_key(sk), rlk)
    bs = []
    for g in BENCH10["cts_groups"]:
        bs.append(Bootstrapper(e, sk, rlk, cts_groups=g, share=bs[0] if bs else None))
    trim_bootstrap_keys(bs)
    return e, R, bs


def _transcipher(lib, log_n, nb, seed=3):
    """transcipher of nb sets whose counter wraps inside the run, with every key product and
    every batched plaintext product recorded.  Returns what the assertions need."""
    e, R, bs = _setup(lib, log_n, seed)
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    iv = rng.integers(0, 256, 16, dtype=np.uint8)
    total = nb * R.n_blk
    first = (-int.from_bytes(bytes(iv[12:]), "big") - total // 3) % 2 ** 32  # wraps at block total / 3
    ctrs = T.ctr_blocks(iv, total, first)[:, 12:]
    assert ctrs[total // 3 - 1].tolist() == [255] * 4 and ctrs[total // 3].tolist() == [0] * 4
    msg = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    data = T.ctr_xor(msg, key, iv, first)
    L0 = R.fresh_level(e.max_level, bs)
    levels = R.ctr_key_levels(L0, bs)
    assert levels == R.key_levels(L0, bs)[:-1] + [R.key_levels(L0, bs)[-1] + 1]
    keys = [R.encrypt_round_key(rk, level=v) for rk, v in zip(T.expand_key(key), levels)]
    key_muls, plain_muls = [], []
    key_mul, mpb = R.key_mul, e.multiply_plain_batch
    R.key_mul = lambda a, k: (key_muls.append((a.level, k.level, a.batch, k.batch)), key_mul(a, k))[1]
    e.multiply_plain_batch = lambda ct, pb: (plain_muls.append((ct.level, ct.batch, pb.batch)), mpb(ct, pb))[1]
    tm = {}
    try:
        out, nref = R.transcipher(data, iv, keys, bs, first=first, timings=tm)
    finally:
        del R.key_mul, e.multiply_plain_batch
    return SimpleNamespace(e=e, R=R, bs=bs, L0=L0, levels=levels, out=out, nref=nref, tm=tm, msg=msg, data=data,
                           key=key, iv=iv, first=first, key_muls=key_muls, plain_muls=plain_muls, nb=nb)


def _check_transcipher(t):
    R, S4 = t.R, 4 * t.R.slabs(t.nb)
    assert t.nref == 3
    assert all(c.level == 0 and c.batch == S4 for row in t.out for c in row)
    # every round started at the level schedule() planned from L0 (ARK0 -> L0 - 1)
    sched = R.schedule(t.L0, t.bs)
    assert [lv for _, lv, _ in t.tm["per_round"]] == [lv for _, lv, _ in sched]
    assert t.L0 == 25 and sched[0][1] == t.L0 - 1 and sched[-1][1] == 5
    # ARK0 and the fold are the only batched plaintext products: K10 (batch 4, one level above
    # the one round 10 consumes) first, then K0 (batch 4 at L0) against 4 S plaintexts each
    assert t.plain_muls == [(t.levels[10], 4, S4)] * 32 + [(t.L0, 4, S4)] * 32
    # every key product met its key at the state's level: no level-down of a key, and the last
    # round's key is the folded one (batch 4 S, no cycling) at the level the schedule consumes
    assert len(t.key_muls) == 32 * 10
    assert all(a == k for a, k, _, _ in t.key_muls)
    assert t.key_muls[-32:] == [(sched[-1][1] - R.KEY_OFFSET, t.levels[10] - 1, S4, S4)] * 32
    assert all(kb == 4 for _, _, _, kb in t.key_muls[:-32])
    got = R.decrypt_blocks(t.out, t.nb)
    assert np.array_equal(T.ctr_xor(t.data, t.key, t.iv, t.first), t.msg)  # the model, block for block
    assert np.array_equal(got, t.msg)


def test_transcipher_ten_rounds_oracle(oracle_lib):
    _check_transcipher(_transcipher(oracle_lib, 10, nb=2))


def test_fold_needs_the_key_one_level_up(oracle_lib):
    """keys[10] at key_levels' level (not ctr_key_levels') leaves no level for the fold: refused
    before anything runs."""
    e = Engine(log_n=10, max_level=30, seed=1, _lib=oracle_lib, special_primes=4, scale_bits=40)
    sk = e.create_secret_key(1)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), None)
    bs = [SimpleNamespace(bits_level=17, stc_bits=[0] * 3), SimpleNamespace(bits_level=19, stc_bits=[0] * 3)]
    lv = R.key_levels(25, bs)
    assert R.ctr_key_levels(25, bs) == lv[:-1] + [lv[-1] + 1]
    keys = [[[SimpleNamespace(level=v)]] for v in lv]
    with pytest.raises(ValueError, match="ctr_key_levels"):
        R.keystream_aes128(bytes(16), 1, keys, bs, data=np.zeros((1, R.n_blk, 16), np.uint8))
    with pytest.raises(ValueError, match="data must be"):
        R.keystream_aes128(bytes(16), 2, keys, bs, data=np.zeros((1, R.n_blk, 16), np.uint8))


# ------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, dict(special_primes=10, digit_primes=12, scale_bits=40)], ids=["K8", "K10A12"])
def test_ctr_reduced_pipeline_bit_exact_vs_oracle(product_lib, oracle_lib, gpu_available, kw):
    """ARK0 by counter planes -> one middle round -> the final round under the data-folded key,
    at N = 2^12: all 32 outputs residue-equal to the oracle's (whose plaintext products run per
    element through aesfhe_mul_pt), and they decrypt to the plain model of that pipeline.  The
    chain holds the 1 + 7 + 5 levels the pipeline uses (two key-switch digits either way)."""
    nb = 6
    rng = np.random.default_rng(3)
    rks = T.expand_key(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + bytes.fromhex("fffff800")
    first = 100  # the counter wraps at block 1948 of the 3072
    data = rng.integers(0, 256, (nb, (1 << 11) // 4, 16), dtype=np.uint8)
    outs = []
    for lib in (product_lib, oracle_lib):
        e = Engine(log_n=12, max_level=13, seed=21, _lib=lib, **dict(dict(special_primes=8), **kw))
        sk = e.create_secret_key(3)
        R = AESSlicedRound(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
        L = e.max_level
        S = R.counter_state(R.encrypt_round_key(rks[0], level=L), iv, nb, first)
        assert all(c.level == L - 1 and c.batch == 8 for row in S for c in row)
        S = R.round(S, R.encrypt_round_key(rks[1], level=L - 1 - R.KEY_OFFSET))
        lk = S[0][0].level - R.KEY_OFFSET  # the level the final round's key product consumes
        K = R.fold_data_key(R.encrypt_round_key(rks[10], level=lk + 1), data)
        assert all(c.level == lk and c.batch == 8 for row in K for c in row)
        S = R.final_round(S, K)
        assert all(c.level == lk - 1 for row in S for c in row)
        ctr = T.ctr_blocks(iv, nb * R.n_blk, first).reshape(nb, R.n_blk, 16)
        want = T.shift_rows(T.sub_bytes(T.aes_round(ctr ^ rks[0], rks[1]))) ^ rks[10] ^ data
        assert np.array_equal(R.decrypt_blocks(S, nb), want)
        outs.append((e, S))
    (g, sg), (o, so) = outs
    for rg, ro in zip(sg, so):
        for cg, co in zip(rg, ro):
            assert np.array_equal(g.export_residues(cg), o.export_residues(co))


@pytest.mark.gpu
def test_transcipher_full_params(product_lib, gpu_available):
    """N = 2^16, L = 30, the bench's ten-round settings, one slab (4 sets, 32 768 blocks)."""
    t = _transcipher(product_lib, 16, nb=4)
    assert t.e._lib.backend == "hip-gfx950"
    _check_transcipher(t)
    margin = t.R.bit_margin(t.out)
    print(f"transcipher N=2^16 nb=4: bit_margin {margin:.4f}, rounds {t.tm['rounds']:.2f} s, "
          f"bootstrap {t.tm['bootstrap']:.2f} s")
    assert margin < 1.0

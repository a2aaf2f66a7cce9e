"""The AES key bundle: the 11 round keys packed into the coefficients of ONE
ciphertext (AESSlicedRound.pack_round_keys / encrypt_key_bundle) and unpacked on the server into
the 11 x 4 x 8 batch-4 key ciphertexts of encrypt_round_key (expand_round_keys, Engine.expand).

CPU: layout, structure, levels and decrypted signs on the oracle, and a reduced CTR pipeline run
under bundle-expanded keys.  GPU: expand_round_keys on the HIP engine is residue-identical to the
oracle's path."""
import numpy as np
import pytest

from aes_xor_fhe import aes_tables as T
from aes_xor_fhe.aes_round_bits import AESSlicedRound
from aes_xor_fhe.fhe import Engine

LEVELS = [4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 3]


def _round_keys(seed):
    return T.expand_key(np.random.default_rng(seed).integers(0, 256, 16, dtype=np.uint8))


def _setup(lib, log_n, max_level=5, seed=41, rlk=False, **kw):
    e = Engine(_lib=lib, log_n=log_n, max_level=max_level, seed=seed,
               **dict(dict(special_primes=2, scale_bits=40), **kw))
    sk = e.create_secret_key(5)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk) if rlk else None)
    return e, R


def _check_structure(keys, levels):
    assert len(keys) == 11
    for k, key in enumerate(keys):
        assert len(key) == 4 and all(len(row) == 8 for row in key)
        for row in key:
            for c in row:
                assert (c.batch, c.npoly, c.level) == (4, 2, levels[k]), (k, c)


# ------------------------------------------------------------------------------------------------
# CPU
def test_pack_round_keys_layout(oracle_lib):
    e, R = _setup(oracle_lib, 11)
    rks = _round_keys(1)
    co = R.pack_round_keys(rks, level=3)
    assert co.shape == (1, 2048) and co.dtype == np.int64
    delta = R.bundle_amplitude(3)
    assert delta == int(round(e.scales[3] * 8))  # 2^10 above Delta / 2^7 (the second stage doubles seven times)
    assert set(np.unique(co)) <= {-delta, delta, 0}
    for k in range(16):  # key k sits at the indices = k mod 16; slots 11..15 stay empty
        part = co[0, k::16]
        if k >= 11:
            assert not part.any()
            continue
        bits = np.array([(int(rks[k][r + 4 * c]) >> j) & 1 for r in range(4) for j in range(8) for c in range(4)])
        assert np.array_equal(part, delta * (1 - 2 * bits))
    assert R.bundle_index(10, 3, 7, 3) == 2047 - 5 and R.bundle_index(3, 0, 0, 0) == 3


def test_bundle_needs_2048_coefficients(oracle_lib):
    e, R = _setup(oracle_lib, 10)
    for call in (lambda: R.pack_round_keys(_round_keys(1)), lambda: R.encrypt_key_bundle(_round_keys(1)),
                 R.create_key_expansion_keys):
        with pytest.raises(ValueError, match="2048 coefficients"):
            call()


def test_expanded_keys_are_the_round_keys(oracle_lib):
    """Structure 11 x 4 x 8, batch 4, the non-uniform levels; every slot of every element decrypts
    to the sign of its key bit, as encrypt_round_key's do."""
    e, R = _setup(oracle_lib, 11)
    rks = _round_keys(2)
    bundle = R.encrypt_key_bundle(rks, level=5)  # one above the highest key
    assert (bundle.batch, bundle.level, bundle.npoly) == (1, 5, 2)
    keys = R.expand_round_keys(bundle, R.create_key_expansion_keys(), LEVELS)
    _check_structure(keys, LEVELS)
    worst = 0.0
    for k, key in enumerate(keys):
        direct = R.encrypt_round_key(rks[k], level=LEVELS[k])
        for r in range(4):
            for j in range(8):
                v = np.real(e.decrypt(key[r][j], R.sk))
                want = np.array([1.0 - 2.0 * ((int(rks[k][r + 4 * c]) >> j) & 1) for c in range(4)])
                assert np.array_equal(np.sign(v), np.broadcast_to(want[:, None], v.shape)), (k, r, j)
                assert np.array_equal(np.sign(np.real(e.decrypt(direct[r][j], R.sk))), np.sign(v))
        worst = max(worst, R.bit_margin(key))
        direct_margin = R.bit_margin(direct)
    print(f"bit_margin of the expanded keys: {worst:.3g} (a directly encrypted key: {direct_margin:.3g})")
    assert worst < 1e-3  # +-1 at a 2^40 scale: the expansion's noise is far below a bit
    with pytest.raises(ValueError, match="11 expansion keys"):
        R.expand_round_keys(bundle, R.create_key_expansion_keys()[:4], LEVELS)
    with pytest.raises(ValueError, match="level"):
        R.expand_round_keys(bundle, R.create_key_expansion_keys(), [5] * 11)  # no level left above the keys


def test_bundle_keys_drive_a_reduced_ctr_pipeline(oracle_lib):
    """ARK0 by counter planes -> one middle round -> the final round under the data-folded key
    (tests/test_ctr.py's reduced pipeline), every key taken from one expanded bundle: the state
    decrypts to the plain model of that pipeline."""
    nb = 2
    rng = np.random.default_rng(3)
    rks = _round_keys(3)
    iv = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + bytes.fromhex("fffffe00")
    first = 100
    # the 1 + 7 + 5 levels the pipeline uses; four special primes keep the oracle's round short
    e, R = _setup(oracle_lib, 11, max_level=14, seed=21, rlk=True, special_primes=4)
    L = e.max_level - 1  # the bundle sits one level above the highest key
    data = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    l1 = L - 1 - R.KEY_OFFSET
    lk = L - 1 - 7 - R.KEY_OFFSET  # a round is 7 levels deep
    levels = [L, l1] + [0] * 8 + [lk + 1]
    keys = R.expand_round_keys(R.encrypt_key_bundle(rks, level=L + 1), R.create_key_expansion_keys(), levels)
    _check_structure(keys, levels)
    S = R.counter_state(keys[0], iv, nb, first)
    S = R.round(S, keys[1])
    assert S[0][0].level - R.KEY_OFFSET == lk
    S = R.final_round(S, R.fold_data_key(keys[10], data))
    ctr = T.ctr_blocks(iv, nb * R.n_blk, first).reshape(nb, R.n_blk, 16)
    want = T.shift_rows(T.sub_bytes(T.aes_round(ctr ^ rks[0], rks[1]))) ^ rks[10] ^ data
    assert np.array_equal(R.decrypt_blocks(S, nb), want)


# ------------------------------------------------------------------------------------------------
# GPU: residues
def _same(g, o, a, b, what):
    x, y = g.export_residues(a), o.export_residues(b)
    assert x.shape == y.shape, what
    if not np.array_equal(x, y):
        raise AssertionError(f"{what}: residues differ; first at [batch, poly, limb, coeff] = {np.argwhere(x != y)[0].tolist()}")


@pytest.mark.gpu
def test_expand_round_keys_residue_exact(product_lib, oracle_lib, gpu_available):
    """N = 2^12: all 11 keys, non-uniform levels."""
    rks = _round_keys(4)
    out = []
    for lib in (product_lib, oracle_lib):
        e, R = _setup(lib, 12)
        keys = R.expand_round_keys(R.encrypt_key_bundle(rks, level=5), R.create_key_expansion_keys(), LEVELS)
        _check_structure(keys, LEVELS)
        out.append((e, keys))
    (g, kg), (o, ko) = out
    for k in range(11):
        for r in range(4):
            for j in range(8):
                _same(g, o, kg[k][r][j], ko[k][r][j], f"key {k} row {r} bit {j}")


@pytest.mark.gpu
def test_one_key_subtree_residue_exact_n16(product_lib, oracle_lib, gpu_available):
    """N = 2^16, L = 6: key 10's subtree alone -- its element of the 16 brought to level 4, steps
    4..10 into 128 elements there, rescaled to level 3."""
    import gc
    rks = _round_keys(5)
    out = []
    for lib in (product_lib, oracle_lib):
        e, R = _setup(lib, 16, max_level=6, special_primes=3)
        xk = R.create_key_expansion_keys()
        by_key = e.expand(R.encrypt_key_bundle(rks, level=6), xk[:4])
        x = R.expand_key_subtree(e.slice(by_key, 10, 1), xk, 3, 6)
        assert (x.batch, x.level) == (128, 3)
        out.append((e, R, by_key, x))
    (g, Rg, bg, xg), (o, _, bo, xo) = out
    _same(g, o, bg, bo, "the 16 per-key elements")
    _same(g, o, xg, xo, "key 10's 128 elements")
    v = np.real(g.decrypt(g.slice(xg, 4 * (3 * 8 + 7), 4), Rg.sk))
    want = np.array([1.0 - 2.0 * ((int(rks[10][3 + 4 * c]) >> 7) & 1) for c in range(4)])
    assert np.array_equal(np.sign(v), np.broadcast_to(want[:, None], v.shape))
    del out, bg, xg, bo, xo, Rg, R, xk, by_key, x
    gc.collect()
    g.pool_trim()

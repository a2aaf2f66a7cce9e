"""Transciphering to numbers: the AES schedule with a level tail
(`out_level`), AESSlicedRound.values_from_bits / decode_values / transcipher_values.

CPU: the schedule on stub bootstrappers, the bit -> value combination on freshly encrypted bits
(all widths, both byte orders, the element / slot map), and a reduced CTR pipeline with a tail on
the oracle.  GPU: that pipeline residue-exact against the oracle at N = 2^12, and one whole
transcipher_values at N = 2^16, L = 30."""
from types import SimpleNamespace

import numpy as np
import pytest

from aes_xor_fhe import aes_tables as T
from aes_xor_fhe.aes_round_bits import AESSlicedRound
from aes_xor_fhe.fhe import Engine
from test_ctr import _setup

STC = 3


def _stubs(levels):
    return [SimpleNamespace(bits_level=v, stc_bits=[0] * STC) for v in levels]


def _bare():
    return AESSlicedRound.__new__(AESSlicedRound)  # the schedule reads class constants only


# ------------------------------------------------------------------------------------------------
# the schedule
@pytest.mark.parametrize("L,levels", [(30, (19,)), (30, (17, 19)), (35, (19,))], ids=["L30-19", "L30-17-19", "L35-19"])
def test_schedule_with_a_level_tail(L, levels):
    R, bss = _bare(), _stubs(levels)
    base = R.schedule(L, bss)
    assert base == R.schedule(L, bss, out_level=0)
    assert R.key_levels(L, bss) == R.key_levels(L, bss, out_level=0)
    assert R.ctr_key_levels(L, bss) == R.ctr_key_levels(L, bss, out_level=0)
    assert R.fresh_level(L, bss) == R.fresh_level(L, bss, out_level=0)
    assert base[-1][1] - R.FINAL_DEPTH == 0  # today's schedule lands on level 0
    for t in (2, 5):
        sched = R.schedule(L, bss, out_level=t)
        assert [r for r, _, _ in sched] == list(range(1, 11))
        end = L - 1  # AddRoundKey(k_0) output
        for rnd, lvl, b in sched:
            depth = R.FINAL_DEPTH if rnd == 10 else R.ROUND_DEPTH
            if b is None:
                assert lvl == end
            else:
                assert end >= STC, f"round {rnd}: the refresh starts at level {end}, SlotToCoeff needs {STC}"
                assert b in bss and lvl == b.bits_level
            assert lvl >= depth, f"round {rnd} at level {lvl}"
            end = lvl - depth
        assert end >= t
        # the tail costs at most the one refresh that lifts round 10
        nref = sum(b is not None for _, _, b in sched)
        assert nref == sum(b is not None for _, _, b in base) + 1
        kl = R.key_levels(L, bss, out_level=t)
        assert kl == [L] + [lvl - R.KEY_OFFSET for _, lvl, _ in sched]
        assert R.ctr_key_levels(L, bss, out_level=t) == kl[:-1] + [kl[-1] + 1]
        L0 = R.fresh_level(L, bss, out_level=t)
        assert L0 <= L and sum(b is not None for _, _, b in R.schedule(L0, bss, out_level=t)) == nref


def test_impossible_tail_is_refused_before_any_work():
    R, bss = _bare(), _stubs((17, 19))
    assert R.schedule(30, bss, out_level=19 - R.FINAL_DEPTH)[-1][1] == 19
    for fn in (R.schedule, R.key_levels, R.ctr_key_levels, R.fresh_level):
        with pytest.raises(ValueError, match="out_level"):
            fn(30, bss, out_level=19 - R.FINAL_DEPTH + 1)
    # the runs check before they touch a ciphertext: stub keys carry a level and nothing else
    keys = [[[SimpleNamespace(level=v)]] for v in R.ctr_key_levels(25, bss)]
    data = np.zeros((1, 4, 16), np.uint8)
    R.n_blk = 4
    with pytest.raises(ValueError, match="out_level"):
        R.transcipher(data, bytes(16), keys, bss, out_level=15)
    with pytest.raises(ValueError, match="out_level"):
        R.transcipher_values(data, bytes(16), keys, bss, 8, keep_levels=13)
    # keys at the levels of another tail: refused, naming the expected list
    with pytest.raises(ValueError, match="ctr_key_levels") as ei:
        R.transcipher_values(data, bytes(16), keys, bss, 8)
    assert str(R.ctr_key_levels(25, bss, out_level=R.CLEAN_LEVELS)) in str(ei.value)
    with pytest.raises(ValueError, match="width"):
        R.transcipher_values(data, bytes(16), keys, bss, 24)


# ------------------------------------------------------------------------------------------------
# bits -> values
def _values(msg, width, byteorder):
    """The unsigned values of (nb, n_blk, 16) message bytes in message order: value i of a block
    is int.from_bytes(block[i * width / 8: (i + 1) * width / 8], byteorder) (exact in int64)."""
    nby = width // 8
    b = np.asarray(msg, dtype=np.uint8).reshape(msg.shape[0], msg.shape[1], 16 // nby, nby).astype(np.int64)
    place = [nby - 1 - i if byteorder == "big" else i for i in range(nby)]
    v = sum(b[..., i] << (8 * place[i]) for i in range(nby))
    assert int(v[0, 0, 0]) == int.from_bytes(bytes(np.asarray(msg, dtype=np.uint8)[0, 0, :nby]), byteorder)
    return v.astype(np.float64)


def _bound(width, mg):
    """The bits' own deviation is the whole error of an exact combination: every bit off by at
    most mg, weights 2^p summing to 2^width - 1, halved by v = (x + 2^width - 1) / 2; then the
    rounding of the encoding and decoding."""
    return (2.0 ** width - 1.0) * mg / 2.0 + 2.0 ** -20 * 2.0 ** width


@pytest.fixture(scope="module")
def fresh_bits(oracle_lib):
    """Freshly encrypted bits of 5 sets (two slabs, the last one a quarter full) at N = 2^10."""
    e = Engine(_lib=oracle_lib, log_n=10, max_level=2, special_primes=2, scale_bits=40, seed=3)
    sk = e.create_secret_key(1)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), None)
    rng = np.random.default_rng(8)
    nb = 5
    msg = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    msg[0, 0], msg[4, R.n_blk - 1] = 0x00, 0xFF
    msg[2, 5], msg[3, 7] = 0xFF, 0x00
    bits = R.encrypt_blocks(msg)
    assert bits[0][0].batch == 8 and bits[0][0].level == 2
    return SimpleNamespace(e=e, R=R, msg=msg, bits=bits, nb=nb, mg=R.bit_margin(bits))


@pytest.mark.parametrize("byteorder", ["big", "little"])
@pytest.mark.parametrize("width", [8, 16, 32])
def test_values_from_fresh_bits(fresh_bits, width, byteorder):
    f = fresh_bits
    R = f.R
    cts, amp = R.values_from_bits(f.bits, width, byteorder)
    assert amp == 1.0 and len(cts) == 32 // width
    assert all((c.level, c.batch, c.npoly) == (2, 8, 2) for c in cts)  # no level spent
    got = R.decode_values(cts, f.nb, width, amp)
    want = _values(f.msg, width, byteorder)
    assert got.shape == want.shape == (f.nb, R.n_blk, 128 // width)
    err = np.abs(got - want).max()
    print(f"width {width} {byteorder}: bit_margin {f.mg:.3e}, max |decoded - v| {err:.3e}, bound {_bound(width, f.mg):.3e}")
    assert 0 < f.mg < 1e-3
    assert err <= _bound(width, f.mg)
    if width == 8:
        assert np.array_equal(np.rint(got), want)
    else:
        # the other byte order is another message: this comparison sees it
        other = _values(f.msg, width, "little" if byteorder == "big" else "big")
        assert np.abs(got - other).max() > 2.0 ** (width - 8)
    # the centred form: amplitude * (2 v - (2^width - 1)), an odd integer in every slot
    x = R.value_slots(cts[0], width, amp)
    assert np.abs(x - (2 * np.rint((x + 2.0 ** width - 1) / 2) - (2.0 ** width - 1))).max() <= 2 * _bound(width, f.mg)


def test_values_element_slot_map(fresh_bits):
    """Element 4 s + c, slot k of output g holds the value from column c of block k of slab s."""
    f = fresh_bits
    R, sc = f.R, f.R.sc
    flat = np.zeros((2 * sc, 16), dtype=np.uint8)
    flat[:f.nb * R.n_blk] = f.msg.reshape(-1, 16)
    for width, G in ((8, 4), (16, 2), (32, 1)):
        cts, amp = R.values_from_bits(f.bits, width, "big")
        nby = width // 8
        for g, ct in enumerate(cts):
            x = R.value_slots(ct, width, amp)
            for s, c, k in [(0, 0, 0), (0, 3, sc - 1), (1, 2, 17), (1, 1, R.n_blk - 1), (1, 0, R.n_blk)]:
                by = flat[s * sc + k, 4 * c + g * nby: 4 * c + (g + 1) * nby]
                v = int.from_bytes(bytes(by), "big")
                assert abs((x[4 * s + c, k] / amp + 2.0 ** width - 1) / 2 - v) <= _bound(width, f.mg)


def test_values_refusals(fresh_bits):
    f = fresh_bits
    with pytest.raises(ValueError, match="width"):
        f.R.values_from_bits(f.bits, 24)
    with pytest.raises(ValueError, match="byteorder"):
        f.R.values_from_bits(f.bits, 16, "middle")
    low = [[f.e.level_down(c, 0) for c in row[:8]] for row in f.bits]
    with pytest.raises(ValueError, match="level 0 is too low"):
        f.R.values_from_bits(low, 32)
    with pytest.raises(ValueError, match="outputs"):
        f.R.decode_values([low[0][0]], f.nb, 16, 1.0)


# ------------------------------------------------------------------------------------------------
# the reduced CTR pipeline with a tail
TAIL = AESSlicedRound.CLEAN_LEVELS + 1  # the cleaning, and one level for 32-bit values to fit


def _reduced(lib, log_n, nb):
    """ARK0 by counter planes -> one middle round -> the final round under the data-folded key
    (test_ctr's reduced pipeline), every key TAIL levels above where the pipeline alone would
    put it, then clean_bits and values_from_bits for widths 8 and 32."""
    rng = np.random.default_rng(3)
    rks = T.expand_key(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + bytes.fromhex("fffffe00")
    first = 100
    e = Engine(log_n=log_n, max_level=13 + TAIL, seed=21, _lib=lib, special_primes=8 if log_n >= 12 else 4, scale_bits=40)
    sk = e.create_secret_key(3)
    R = AESSlicedRound(e, sk, e.create_public_key(sk), e.create_relinearization_key(sk))
    data = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    L = e.max_level
    S = R.counter_state(R.encrypt_round_key(rks[0], level=L), iv, nb, first)
    S = R.round(S, R.encrypt_round_key(rks[1], level=L - 1 - R.KEY_OFFSET))
    lk = S[0][0].level - R.KEY_OFFSET
    S = R.final_round(S, R.fold_data_key(R.encrypt_round_key(rks[10], level=lk + 1), data))
    assert all(c.level == TAIL for row in S for c in row)
    mg0 = R.bit_margin(S)
    C = R.clean_bits(S)
    assert all(c.level == TAIL - R.CLEAN_LEVELS for row in C for c in row)
    v8, a8 = R.values_from_bits(C, 8, in_scale=2.0)
    v32, a32 = R.values_from_bits(C, 32, in_scale=2.0)
    assert a8 == a32 == 2.0 and all(c.level == TAIL - R.CLEAN_LEVELS for c in v8 + v32)
    ctr = T.ctr_blocks(iv, nb * R.n_blk, first).reshape(nb, R.n_blk, 16)
    want = T.shift_rows(T.sub_bytes(T.aes_round(ctr ^ rks[0], rks[1]))) ^ rks[10] ^ data
    return SimpleNamespace(e=e, R=R, nb=nb, bits=C, v8=v8, v32=v32, want=want, mg0=mg0, mg=R.bit_margin(C, scale=2.0))


def _check_reduced(p):
    R = p.R
    assert np.array_equal(R.decrypt_blocks(p.bits, p.nb), p.want)
    got8 = R.decode_values(p.v8, p.nb, 8, 2.0)
    got32 = R.decode_values(p.v32, p.nb, 32, 2.0)
    e8, e32 = np.abs(got8 - p.want).max(), np.abs(got32 - _values(p.want, 32, "big")).max()
    print(f"reduced pipeline: bit_margin {p.mg0:.3e} -> cleaned {p.mg:.3e}; max |decoded - v| width 8 {e8:.3e}, "
          f"width 32 {e32:.3e} (bound {_bound(32, p.mg):.3e})")
    assert np.array_equal(np.rint(got8), p.want)  # every byte, exactly
    assert e8 <= _bound(8, p.mg) and e32 <= _bound(32, p.mg)


def test_reduced_ctr_pipeline_with_tail_oracle(oracle_lib):
    _check_reduced(_reduced(oracle_lib, 10, nb=5))


@pytest.mark.gpu
def test_reduced_ctr_pipeline_with_tail_vs_oracle(product_lib, oracle_lib, gpu_available):
    g, o = _reduced(product_lib, 12, nb=6), _reduced(oracle_lib, 12, nb=6)
    assert g.e._lib.backend == "hip-gfx950"
    _check_reduced(g)
    for cg, co in zip([c for row in g.bits for c in row] + g.v8 + g.v32, [c for row in o.bits for c in row] + o.v8 + o.v32):
        assert np.array_equal(g.e.export_residues(cg), o.e.export_residues(co))


@pytest.mark.gpu
def test_transcipher_values_full_params(product_lib, gpu_available):
    """N = 2^16, L = 30, the bench's ten-round settings, one slab (4 sets, 32 768 blocks)."""
    nb = 4
    e, R, bs = _setup(product_lib, 16)
    assert e._lib.backend == "hip-gfx950"
    rng = np.random.default_rng(3)
    key, iv = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, 16, dtype=np.uint8)
    msg = rng.integers(0, 256, (nb, R.n_blk, 16), dtype=np.uint8)
    first = 9
    data = T.ctr_xor(msg, key, iv, first)
    t = R.CLEAN_LEVELS
    L0 = R.fresh_level(e.max_level, bs, out_level=t)
    sched = R.schedule(L0, bs, out_level=t)
    keys = [R.encrypt_round_key(rk, level=v) for rk, v in zip(T.expand_key(key), R.ctr_key_levels(L0, bs, out_level=t))]
    seen = []
    vfb = R.values_from_bits
    R.values_from_bits = lambda bits, *a, **k: (seen.append(bits), vfb(bits, *a, **k))[1]
    try:
        cts, amp, nref = R.transcipher_values(data, iv, keys, bs, 8, first=first)
    finally:
        del R.values_from_bits
    out_level = sched[-1][1] - R.FINAL_DEPTH - R.CLEAN_LEVELS
    assert nref == sum(b is not None for _, _, b in sched)
    assert amp == 2.0 and len(cts) == 4 and all(c.level == out_level and c.batch == 4 for c in cts)
    assert len(seen) == 1
    mg = R.bit_margin(seen[0], scale=2.0)
    got8 = R.decode_values(cts, nb, 8, amp)
    v32, a32 = R.values_from_bits(seen[0], 32, in_scale=2.0)
    got32 = R.decode_values(v32, nb, 32, a32)
    e8, e32 = np.abs(got8 - msg).max(), np.abs(got32 - _values(msg, 32, "big")).max()
    print(f"transcipher_values N=2^16 nb=4: {nref} refreshes, output level {out_level}, cleaned bit_margin {mg:.3e}, "
          f"max |decoded - v| width 8 {e8:.3e}, width 32 {e32:.3e} (bound {_bound(32, mg):.3e})")
    assert np.array_equal(np.rint(got8), msg)
    assert v32[0].level == out_level and e32 <= _bound(32, mg)

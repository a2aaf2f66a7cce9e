"""Residue parity of every fused key-switch shape at N = 2^16.

Which kernels a key switch runs at N = 2^16 is decided on the host by (K special primes, digit
width A, level l, rescale depth r): ModUp of a digit of alpha limbs is k_bconv_cols<ceil(alpha / 4),
true, false> (a one-limb digit: the spread column kernel, or k_bconv_cols<1> when a row pass follows
-- hoisted rotations), ModDown is k_bconv_cols<ceil((K + r + 1) / 4), true, true> with the exact
conversion's v in slot K + r while K + r + 1 <= 16, the unfused conversion above that, and separate
relinearise + rescale steps when K + r > 16 (csrc/bconv_cols.h, engine.hip ks_modup /
ks_finish_fused / moddown_acc / relin_rescale).  Targets go in tiles of 4 (nt % 4 partial tiles).
The fused kernels run at no other size, and the other suites reach K = 3, 8, 10 at a few levels.

Here, residue for residue against the CPU oracle (np.array_equal on export_residues), on seeded
uniformly random residues brought in with import_residues (the arithmetic is exact integer work,
so the inputs need not be encryptions; keys come from identical seeds on both engines):

* Part A: a matrix of (K, A, L, B) engines that reaches NSTEP 1..4 of both instantiations, all
  fifteen v-slot positions, every nt % 4, odd and even batches and both fallback boundaries, every
  op at every level;
* Part B: ModUp sources y = [x qhat^{-1}]_q chosen as extreme words (0, q - 1, 0xFF / 0x80 / 0x7F
  byte runs, alternating 0 and q - 1 across slots) for the `^ 0x80808080` bias and the corr table;
* Part C: the bench chain (L = 30, K = 10, A = 12) at every level 1..30, and the S-box's own
  poly2_int call (batch 4, 8 outputs: the relinearisation at l = 26 with batch 32 through
  k_bconv_cols<4, true, true>);
* Part D: around every GPU op the engine's launch profile is read and the launches per class are
  compared with ks_plan(), a pure function (_ks_helpers.py, CPU-tested against hand-written values): the
  test proves which path ran, not only that some path gave the right residues;
* Part E (CPU): the input builders and the ops' result levels / batches on the oracle alone.
"""
import math

import numpy as np
import pytest

from aes_xor_fhe.fhe import Engine

# the helpers and ks_plan (Part D's restated dispatch) are shared with test_range_bounds.py
from _ks_helpers import (NHOIST, OPS, RESCALES, _check_construction, _check_path, _compare, _drop,  # noqa: E402
                         _expect_out, _extreme_ct, _keys, _ops_at, _pair, _pool, _profiled, _run_op, _sweep,
                         ks_plan)


# id -> K, A, L, batch, levels (None: every level 1..L)
SHAPES = {
    "K1": dict(K=1, A=1, L=4, B=3, levels=None),
    "K4": dict(K=4, A=4, L=6, B=3, levels=None),
    "K7": dict(K=7, A=7, L=8, B=3, levels=None),
    "K10A12B1": dict(K=10, A=12, L=13, B=1, levels=None),
    "K10A12B3": dict(K=10, A=12, L=13, B=3, levels=None),
    "K10A12B8": dict(K=10, A=12, L=13, B=8, levels=None),
    "K13": dict(K=13, A=13, L=14, B=3, levels=None),
    "K14": dict(K=14, A=14, L=5, B=3, levels=None),
    "K16": dict(K=16, A=16, L=17, B=1, levels=(15, 16, 17)),
}
BENCH = dict(K=10, A=12, L=30)
# the bench chain's levels in groups of at most ~15 s of oracle time each; every level 1..30 once
LEVEL_GROUPS = {"l01-08": range(1, 9), "l09-14": range(9, 15), "l15-19": range(15, 20),
                "l20-23": range(20, 24), "l24-27": range(24, 28), "l28-30": range(28, 31)}


def _kw(K, A, L, seed=77):
    return dict(log_n=16, max_level=L, special_primes=K, digit_primes=A, scale_bits=40, seed=seed)


def coverage(shape):
    """(NSTEP, VC) pairs, v-slot positions and nt % 4 values one matrix row reaches (ks_plan)."""
    s = SHAPES[shape]
    pairs, vslots, ntmod = set(), set(), set()
    for l in s["levels"] or range(1, s["L"] + 1):
        for op in OPS:
            if (op in ("multiply", "multiply_bcast", "multiply_fma", "poly2_int") and l < 2) or \
                    (op == "multiply_bcast" and s["B"] == 1):
                continue
            p = ks_plan(s["K"], s["A"], l, RESCALES[op], op)
            pairs |= {(n, False) for n in p["modup_nstep"]}
            ntmod |= {nt % 4 for nt in p["modup_nt"]}
            if p["moddown_cols"]:
                pairs.add((p["moddown_nstep"], True))
                vslots.add(p["vslot"])
                ntmod.add(p["moddown_nt"] % 4)
    return sorted(pairs), sorted(vslots), sorted(ntmod)


def test_ks_plan_bench_chain_hand_values():
    """ks_plan against values written by hand from engine.hip for the bench chain (K = 10,
    A = 12), and the coverage the matrix is there for."""
    K, A = 10, 12
    p = ks_plan(K, A, 30, 0, "relinearize")
    assert p["digits"] == [12, 12, 7] and p["modup_cols"] == 3 and p["modup_nstep"] == [2, 3]
    assert p["modup_nt"] == [29, 29, 34] and p["spread"] == 0
    assert (p["moddown_cols"], p["moddown"], p["moddown_nstep"], p["vslot"], p["moddown_nt"]) == (1, 0, 3, 10, 31)
    assert p["finish"] == "ks_rows_fin.ks"
    p = ks_plan(K, A, 30, 1, "multiply")
    assert (p["moddown_nstep"], p["vslot"], p["moddown_nt"], p["finish"]) == (3, 11, 30, "ks_rows_fin.prod")
    p = ks_plan(K, A, 30, 2, "poly2_int")
    assert (p["moddown_nstep"], p["vslot"], p["moddown_nt"], p["finish"]) == (4, 12, 29, "ks_rows_fin.ks")
    assert not p["separate"]
    # l = 24: 25 limbs, the last digit one limb wide -- spread for ops 1-5, k_bconv_cols<1> hoisted
    p = ks_plan(K, A, 24, 0, "rotate")
    assert p["digits"] == [12, 12, 1] and p["modup_cols"] == 2 and p["spread"] == 1 and p["modup_nstep"] == [3]
    p = ks_plan(K, A, 24, 0, "rotate_hoisted")
    assert p["modup_cols"] == 3 and p["spread"] == 0 and p["modup_nstep"] == [1, 3]
    assert p["modup_nt"] == [23, 23, 34] and p["moddown_cols"] == NHOIST and p["finish"] == "ntt_fwd_rows_fin"
    p = ks_plan(K, A, 23, 1, "multiply_fma")
    assert p["digits"] == [12, 12] and p["modup_cols"] == 2 and p["spread"] == 0 and p["moddown_nt"] == 23
    p = ks_plan(K, A, 11, 2, "poly2_int")
    assert p["digits"] == [12] and p["modup_cols"] == 1 and p["modup_nt"] == [10] and p["moddown_nt"] == 10
    # the fallback boundaries: 17 slots unfused with combined tables (K = 14, r = 2); K = 16
    p = ks_plan(14, 14, 5, 2, "poly2_int")
    assert (p["separate"], p["moddown_cols"], p["moddown"], p["moddown_nt"]) == (False, 0, 1, 4)
    assert ks_plan(14, 14, 5, 1, "multiply")["vslot"] == 15
    p = ks_plan(16, 16, 17, 1, "multiply")
    assert (p["separate"], p["moddown_cols"], p["moddown"], p["finish"]) == (True, 0, 1, "ks_rows_fin.ks")
    assert p["rescales"] == 1 and ks_plan(16, 16, 17, 2, "poly2_int")["rescales"] == 2
    assert ks_plan(14, 14, 5, 2, "poly2_int")["rescales"] == 0
    assert p["digits"] == [16, 2] and p["modup_nstep"] == [1, 4]
    assert ks_plan(16, 16, 15, 0, "rotate")["moddown"] == 1
    # what the matrix reaches: NSTEP 1..4 of both instantiations, the fifteen v slots, every nt % 4
    pairs, vslots, ntmod = set(), set(), set()
    for s in SHAPES:
        a, b, c = coverage(s)
        pairs |= set(a)
        vslots |= set(b)
        ntmod |= set(c)
    assert pairs == {(n, vc) for n in (1, 2, 3, 4) for vc in (False, True)}
    assert vslots == set(range(1, 16)) and ntmod == {0, 1, 2, 3}
    # K13: one digit of l + 1 limbs up to l = 12 (NSTEP 1..4), then (13, 1) and (13, 2)
    assert coverage("K13")[0] == [(1, False), (2, False), (3, False), (4, False), (4, True)]
    assert coverage("K13")[1] == [13, 14, 15] and coverage("K10A12B8")[1] == [10, 11, 12]
    assert coverage("K16")[:2] == ([(1, False), (4, False)], [])  # no fused ModDown at K = 16
    assert sorted(l for g in LEVEL_GROUPS.values() for l in g) == list(range(1, 31))


# ------------------------------------------------------------------------------------------------
# Part A: the shape matrix
@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("ident", list(SHAPES))
def test_keyswitch_shape_matrix_bit_exact(product_lib, oracle_lib, gpu_available, ident):
    s = SHAPES[ident]
    K, A, L, B = s["K"], s["A"], s["L"], s["B"]
    g, o = _pair(product_lib, oracle_lib, **_kw(K, A, L))
    try:
        assert g.digit_primes == A and g.special_prime_count == K
        kg, ko = _keys(g), _keys(o)
        pool = _pool(g.primes, L, B, 6, seed=1000 + K)
        _sweep(g, o, kg, ko, ident, K, A, B, s["levels"] or range(1, L + 1), pool)
    finally:
        kg = ko = None
        _drop(g, o)


# ------------------------------------------------------------------------------------------------
# Part B: extreme ModUp source words
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("ident,l", [("K10A12B1", 13), ("K13", 14)], ids=["K10A12-l13", "K13-l14"])
def test_modup_extreme_source_words_bit_exact(product_lib, oracle_lib, gpu_available, ident, l):
    s = SHAPES[ident]
    K, A = s["K"], s["A"]
    g, o = _pair(product_lib, oracle_lib, **_kw(K, A, s["L"]))
    try:
        kg, ko = _keys(g), _keys(o)
        arr, want = _extreme_ct(o, A, l, seed=500 + K)
        co = _check_construction(o, arr, want)
        what = f"engine {ident} (extreme source words), op relinearize, level {l}, batch 1"
        og, prof = _profiled(g, lambda: [g.relinearize(g.import_residues(arr), kg["rlk"])])
        _check_path(prof, K, A, l, "relinearize", what)
        _compare(g, o, og, [o.relinearize(co, ko["rlk"])], _expect_out("relinearize", l, 1), what)
        del og, co
    finally:
        kg = ko = None
        _drop(g, o)


# ------------------------------------------------------------------------------------------------
# Part C: the bench chain
@pytest.fixture(scope="module")
def bench_pair(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **_kw(BENCH["K"], BENCH["A"], BENCH["L"], seed=5))
    st = dict(g=g, o=o, kg=_keys(g), ko=_keys(o), pool=_pool(g.primes, BENCH["L"], 1, 6, seed=2030))
    yield st
    st.clear()
    _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("group", list(LEVEL_GROUPS))
def test_bench_chain_level_sweep_bit_exact(bench_pair, group):
    st = bench_pair
    _sweep(st["g"], st["o"], st["kg"], st["ko"], "bench-chain", BENCH["K"], BENCH["A"], 1, LEVEL_GROUPS[group],
           st["pool"])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_chain_sbox_poly2_int_bit_exact(bench_pair):
    """The round's S-box call: poly2_int(x^1..x^15, y^1..y^15, 64 W, 64, rlk, slab_rot = 1) at
    batch 4 with the power basis's levels 30 - ceil(log2 k) -- 8 outputs, so the relinearisation
    runs at l = 26 with batch 32 and r = 2: k_bconv_cols<4, true, true>, v in slot 12."""
    from aes_xor_fhe.aes_round_bits import walsh_sbox
    st = bench_pair
    g, o = st["g"], st["o"]
    W = np.rint(walsh_sbox() * 64).astype(np.int64)
    assert W.shape == (8, 16, 16)
    levels = [30 - math.ceil(math.log2(k)) for k in range(1, 16)]
    assert min(levels) == 26
    base = _pool(g.primes, BENCH["L"], 4, 4, seed=2031)  # polys 0-1: x, 2-3: y; power k: rolled by k
    what = "engine bench-chain, op poly2_int (S-box weights, slab_rot 1), level 26, batch 4"

    def run(eng, k):
        xb = [eng.import_residues(np.roll(base[:, 0:2, :lv + 1], 17 * i, axis=-1)) for i, lv in enumerate(levels)]
        yb = [eng.import_residues(np.roll(base[:, 2:4, :lv + 1], 29 * i, axis=-1)) for i, lv in enumerate(levels)]
        return eng.poly2_int(xb, yb, W, 64, k["rlk"], slab_rot=1)

    og, prof = _profiled(g, lambda: run(g, st["kg"]))
    _check_path(prof, BENCH["K"], BENCH["A"], 26, "poly2_int", what)
    assert ks_plan(BENCH["K"], BENCH["A"], 26, 2, "poly2_int")["moddown_nstep"] == 4
    oo = run(o, st["ko"])
    _compare(g, o, og, oo, [(24, 4, False)] * 8, what)


# ------------------------------------------------------------------------------------------------
# Part E: the plumbing on the oracle alone (CPU)
@pytest.mark.timeout(300)
@pytest.mark.parametrize("ident", ["K1", "K4", "K14"])
def test_plumbing_on_the_oracle(oracle_lib, ident):
    """The input builders and every op's result levels and batches, without a GPU: import ->
    export round-trips, levels are (l, l - 1, l - 2), poly2_int gives two live outputs of batch B
    around the zero ciphertext."""
    s = SHAPES[ident]
    K, A, L, B = s["K"], s["A"], s["L"], s["B"]
    o = Engine(_lib=oracle_lib, **_kw(K, A, L))
    assert o.digit_primes == A and o.special_prime_count == K and o.max_level == L
    ko = _keys(o)
    pool = _pool(o.primes, L, B, 6, seed=1000 + K)
    assert all(int(pool[:, :, i].max()) < o.primes[i] for i in range(L + 1))
    for l in (1, 2, L):
        arr = pool[:, 3:6, :l + 1]
        ct = o.import_residues(arr)
        assert (ct.level, ct.batch, ct.npoly) == (l, B, 3)
        assert np.array_equal(o.export_residues(ct), arr)
        assert _ops_at(l, B) == [op for op in OPS if l >= 2 or RESCALES[op] == 0]
        for op in _ops_at(l, B):
            outs = _run_op(o, ko, op, pool, l)
            got = [(c.level, c.batch, c.is_zero) for c in outs]
            assert got == _expect_out(op, l, B), (ident, op, l, got)
            assert all(c.npoly == 2 for c in outs)
            if op == "poly2_int":
                assert not o.export_residues(outs[1]).any() and o.export_residues(outs[0]).any()
    # the extreme-word construction (Part B) on this chain's top level
    arr, want = _extreme_ct(o, A, L, seed=500 + K)
    _check_construction(o, arr, want)

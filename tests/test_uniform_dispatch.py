"""Residue parity of the key-switch row kernels' two bodies (csrc/ks_fused.h).

k_nttf_rows_ks_p branches once per workgroup on q >= 2^42 into a body with the big-prime folds
inline or a body with none, the product prologue takes the multiply-add's operand presence (fac,
pc) as template arguments, the FIN epilogue tests its addend once per component, and the fused base
conversion (csrc/bconv_cols.h) runs an unguarded conversion loop on full tiles.  Which body a limb
takes depends on its prime alone, so three short chains (L = 4, K = A = 2, N = 2^16) put every limb
on one side, every limb on the other, and the bench chain's mixture:

    chain   base  special  scale   limb bits (Q | P)
    small    41     41      40     41 41 40 40 41 | 41 41    every limb below 2^42 (INV's small body too)
    big      50     50      44     50 45 44 45 45 | 50 50    every limb at or above 2^42
    mixed    50     50      40     50 41 40 40 41 | 50 50    the bench chain's shape

On each chain, at every level 1..4 and batches 1 and 3, residue for residue against the CPU oracle
(_ks_helpers: seeded uniform residues through import_residues, np.array_equal on export_residues):
the product relinearisation with rescale (PROD), multiply_fma with and without the addend
ciphertext (fac, pc), a rotation (plain, r = 0, fin.add present), the relinearisation of a
3-component ciphertext (plain, r = 0) and poly2_int (plain, r = 2), and linear_bsgs with two giants
(the accumulating k_nttf_rows_ks).  Ops with a rescale start at level 2, as everywhere in this
suite (a rescale needs a limb to drop below the result's).  The launch profile proves which fused
kernels ran (ks_plan / _check_path).
"""
import numpy as np
import pytest

from _ks_helpers import (_check_path, _compare, _drop, _expect_out, _keys, _pair, _pool, _profiled,  # noqa: E402
                         _run_op, RESCALES)

K = A = 2
L = 4
BIG = 1 << 42  # kBigPrime
CHAINS = {
    "small": dict(base_bits=41, special_bits=41, scale_bits=40, bits=[41, 41, 40, 40, 41, 41, 41]),
    "big": dict(base_bits=50, special_bits=50, scale_bits=44, bits=[50, 45, 44, 45, 45, 50, 50]),
    "mixed": dict(base_bits=50, special_bits=50, scale_bits=40, bits=[50, 41, 40, 40, 41, 50, 50]),
}
KS_OPS = ("multiply", "multiply_fma", "multiply_fma_noc", "rotate", "relinearize", "poly2_int")


def _kw(chain):
    c = CHAINS[chain]
    return dict(log_n=16, max_level=L, special_primes=K, digit_primes=A, scale_bits=c["scale_bits"],
                base_bits=c["base_bits"], special_bits=c["special_bits"], seed=31)


def _all_primes(eng):
    """The chain's primes, Q then P."""
    ps = list(eng.primes)
    if len(ps) == L + 1:
        ps += list(eng.special_primes)
    return ps


def _op(eng, k, op, pool, l):
    if op == "multiply_fma_noc":  # fac without pc: the FMA prologue's form with no addend ciphertext
        imp = lambda lo, hi: eng.import_residues(pool[:, lo:hi, :l + 1])  # noqa: E731
        return [eng.multiply_fma(imp(0, 2), imp(2, 4), k["rlk"], alpha=3, beta=0.25)]
    return _run_op(eng, k, op, pool, l)


def _plan_op(op):
    return "multiply_fma" if op == "multiply_fma_noc" else op


@pytest.mark.parametrize("chain", list(CHAINS))
def test_chain_limb_classes(oracle_lib, chain):
    """The three chains are what the table says (CPU: the oracle builds the same primes)."""
    from aes_xor_fhe.fhe import Engine
    o = Engine(_lib=oracle_lib, **_kw(chain))
    ps = _all_primes(o)
    assert [p.bit_length() for p in ps] == CHAINS[chain]["bits"][:len(ps)]
    big = [p >= BIG for p in ps]
    assert {"small": not any(big), "big": all(big), "mixed": any(big) and not all(big)}[chain]
    assert o.digit_primes == A and o.special_prime_count == K


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_row_kernel_bodies_bit_exact(product_lib, oracle_lib, gpu_available, chain, B):
    g, o = _pair(product_lib, oracle_lib, **_kw(chain))
    try:
        kg, ko = _keys(g), _keys(o)
        pool = _pool(g.primes, L, B, 6, seed=4100 + B)
        for l in range(1, L + 1):
            for op in KS_OPS:
                if l < 2 and RESCALES[_plan_op(op)] > 0:
                    continue
                what = f"chain {chain}, op {op}, level {l}, batch {B}"
                og, prof = _profiled(g, lambda: _op(g, kg, op, pool, l))
                _check_path(prof, K, A, l, _plan_op(op), what)
                oo = _op(o, ko, op, pool, l)
                _compare(g, o, og, oo, _expect_out(_plan_op(op), l, B), what)
                del og, oo
    finally:
        kg = ko = None
        _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_linear_bsgs_two_giants_bit_exact(product_lib, oracle_lib, gpu_available, chain, B):
    """linear_bsgs with two keyed giants: the first one's accumulators are written by
    k_nttf_rows_ks (which shares the row NTT with the pipelined kernels), the second one adds into
    them in the pipelined kernels' `accum` prologue and finishes the sum."""
    g, o = _pair(product_lib, oracle_lib, **_kw(chain))
    try:
        n = g.slot_count
        rng = np.random.default_rng(77)
        z = rng.uniform(-1, 1, (B, n))
        babies, giants = [0, 1], [2, 4]
        diags = [rng.uniform(-1, 1, n) for _ in range(4)]
        plan = [(d, [(b, 2 * j + b) for b in range(2)]) for j, d in enumerate(giants)]
        for l in range(1, L + 1):
            outs = []
            for eng in (g, o):
                sk = eng.create_secret_key(7)
                c = eng.encrypt(z, eng.create_public_key(sk), level=l)
                bk = [None if d == 0 else eng.create_hoisted_rotation_key(sk, -d) for d in babies]
                gk = [None if d == 0 else eng.create_fixed_rotation_key(sk, -d) for d, _ in plan]
                pts = [eng.encode(v) for v in diags]
                terms = [[(b, pts[i]) for b, i in tl] for _, tl in plan]
                if eng is g:
                    out, prof = _profiled(g, lambda: g.linear_bsgs(c, bk, gk, terms))
                    assert prof.get("ks_rows_acc.ks", 0) >= 1 and prof.get("ks_rows_fin.ks", 0) >= 1, \
                        f"chain {chain}, level {l}: the giants' row passes are missing in {prof}"
                else:
                    out = eng.linear_bsgs(c, bk, gk, terms)
                assert (out.level, out.batch) == (l - 1, B)
                outs.append(eng.export_residues(out))
                del out, c, bk, gk, pts, terms
            assert np.array_equal(outs[0], outs[1]), f"chain {chain}, linear_bsgs, level {l}, batch {B}: residues differ"
    finally:
        _drop(g, o)

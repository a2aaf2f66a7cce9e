"""Exact integer combinations (Engine.lincomb_int / aesfhe_lincomb_int, include/aesfhe_ext.h;
DESIGN.md section 5.3): outs[r] = sum_i w[r][i] cts[i] mod every prime, no rounding, no level.

CPU: the facade's fallback (negate + double-and-add through aesfhe.h, what the oracle runs)
against the sum restated in Python integers.  GPU: the HIP kernel residue-exact against that
fallback on the oracle, its refusals (status and no pool block), and its launch count."""
import ctypes as C

import numpy as np
import pytest

from _int_refs import obj, u64
from _ks_helpers import _drop, _pair, _pool, _profiled
from aes_xor_fhe._abi import c_ct_p
from aes_xor_fhe.aes_round_bits import AESSlicedRound
from aes_xor_fhe.fhe import Engine

EARG, EDEGREE, ELEVEL = -1, -4, -5

# n = 8 inputs, m = 3 outputs: 0, +-1, a weight above 2^40, one above every prime (2^61 + 5 with
# its sign), and input 5's column all zero
W_CPU = [[0, 1, -1, (1 << 40) + 3, -((1 << 61) + 5), 0, 2, -7],
         [1, 0, 0, -1, (1 << 61) + 5, 0, -((1 << 40) + 3), 1],
         [-((1 << 61) + 5), 3, 1, 0, 0, 0, 1, (1 << 40) + 3]]


def lincomb_int_ref(xs, W, primes):
    """The definition in Python integers: xs n arrays (B, P, nl, N) -> m arrays."""
    xo = [obj(x) for x in xs]
    outs = []
    for row in W:
        acc = np.zeros(xo[0].shape, dtype=object)
        for x, w in zip(xo, row):
            acc = acc + int(w) * x
        for i in range(acc.shape[2]):
            acc[:, :, i] %= primes[i]
        outs.append(u64(acc))
    return outs


def _inputs(primes, level, B, npoly, n, seed, N):
    """n distinct residue arrays from one random pool: input i is the pool rolled by 17 i + 1
    coefficients (a limb's words stay below its prime)."""
    base = _pool(primes, level, B, npoly, seed, n=N)
    return [np.ascontiguousarray(np.roll(base, 17 * i + 1, axis=3)) for i in range(n)]


def test_fallback_equals_python_integers_and_one_weight_bites(oracle_lib):
    e = Engine(_lib=oracle_lib, log_n=10, max_level=3, special_primes=2, seed=3)
    assert not e._lib.has_ext  # the oracle runs the composition through aesfhe.h
    assert (1 << 61) + 5 > max(e.primes)
    xs = _inputs(e.primes, 3, 4, 2, 8, seed=11, N=1 << 10)
    cts = [e.import_residues(x) for x in xs]
    outs = e.lincomb_int(cts, W_CPU)
    want = lincomb_int_ref(xs, W_CPU, e.primes[:4])
    assert len(outs) == 3
    for c, w in zip(outs, want):
        assert (c.level, c.batch, c.npoly) == (3, 4, 2)
        assert np.array_equal(e.export_residues(c), w)
    # the inputs are untouched (a lone weight 1 must not hand the input itself back)
    assert all(np.array_equal(e.export_residues(c), x) for c, x in zip(cts, xs))
    one = e.lincomb_int([cts[0]], [[1]])[0]
    assert one is not cts[0] and np.array_equal(e.export_residues(one), xs[0])
    # the comparison bites: one weight off by one is another result, in the reference and in the
    # fallback alike
    W2 = [list(r) for r in W_CPU]
    W2[1][4] += 1
    off = lincomb_int_ref(xs, W2, e.primes[:4])
    assert not np.array_equal(off[1], want[1]) and np.array_equal(off[0], want[0])
    got2 = e.lincomb_int(cts, W2)
    assert not np.array_equal(e.export_residues(got2[1]), want[1])
    assert np.array_equal(e.export_residues(got2[1]), off[1])
    # an all-zero row is a zero ciphertext
    z = e.lincomb_int(cts[:2], [[0, 0], [5, 0]])
    assert z[0].is_zero and not e.export_residues(z[0]).any()
    assert np.array_equal(e.export_residues(z[1]), lincomb_int_ref(xs[:2], [[5, 0]], e.primes[:4])[0])


def test_fallback_refusals(oracle_lib):
    e = Engine(_lib=oracle_lib, log_n=10, max_level=3, special_primes=2, seed=3)
    xs = _inputs(e.primes, 3, 2, 3, 1, seed=5, N=1 << 10)
    a = e.import_residues(xs[0][:, :2])
    with pytest.raises(RuntimeError, match="level error"):
        e.lincomb_int([a, e.import_residues(xs[0][:, :2, :3])], [[1, 1]])
    with pytest.raises(RuntimeError, match="degree error"):
        e.lincomb_int([a, e.import_residues(xs[0])], [[1, 1]])
    with pytest.raises(RuntimeError, match="invalid argument"):
        e.lincomb_int([a, e.import_residues(xs[0][:1, :2])], [[1, 1]])
    with pytest.raises(RuntimeError, match="invalid argument"):
        e.lincomb_int([], [[]])
    with pytest.raises(RuntimeError, match="invalid argument"):
        e.lincomb_int([a] * 33, [[1] * 33])
    with pytest.raises(RuntimeError, match="invalid argument"):
        e.lincomb_int([a], [[1]] * 17)
    with pytest.raises(ValueError):
        e.lincomb_int([a], [[-(1 << 63)]])
    with pytest.raises(ValueError):
        e.lincomb_int([a, a], [[1]])


# ------------------------------------------------------------------------------------------------
# GPU
W_FAN = [[(r + 1) * (-1) ** (r + i) * ((1 << (3 * r + i)) + i) if (r + i) % 5 else 0 for i in range(5)] for r in range(16)]

SHAPES = [
    # log_n, level, batch, npoly, weights
    pytest.param(12, 3, 4, 2, [r[:8] for r in W_CPU] + [[0] * 8], id="N12-l3-B4-8to4-cpu-weights"),
    pytest.param(16, 14, 8, 2, [[-(1 << p) for p in range(32)]], id="N16-l14-B8-32to1"),
    pytest.param(16, 14, 8, 2, [[(1 << 37) + (1 << 7)]], id="N16-l14-B8-1to1-times"),
    pytest.param(12, 3, 4, 2, W_FAN, id="N12-l3-B4-5to16"),
    pytest.param(12, 3, 4, 3, [r[:8] for r in W_CPU], id="N12-l3-B4-8to3-npoly3"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,level,batch,npoly,W", SHAPES)
def test_lincomb_int_residue_exact_vs_oracle(product_lib, oracle_lib, gpu_available, log_n, level, batch, npoly, W):
    kw = dict(log_n=log_n, max_level=level, seed=5, special_primes=2 if log_n == 12 else 8)
    g, o = _pair(product_lib, oracle_lib, **kw)
    assert g._lib.has_ext and not o._lib.has_ext
    n, m = len(W[0]), len(W)
    base = _pool(g.primes, level, batch, npoly, seed=7, n=1 << log_n)
    cg, co = [], []
    for i in range(n):
        x = np.ascontiguousarray(np.roll(base, 17 * i + 1, axis=3))
        cg.append(g.import_residues(x))
        co.append(o.import_residues(x))
    del base, x
    og, prof = _profiled(g, lambda: g.lincomb_int(cg, W))
    assert prof.get("lincomb_int") == 1 and not prof.get("add"), prof
    oo = o.lincomb_int(co, W)
    assert len(og) == len(oo) == m
    for r, (a, b) in enumerate(zip(og, oo)):
        assert (a.level, a.batch, a.npoly) == (b.level, b.batch, b.npoly) == (level, batch, npoly)
        zero = not any(W[r])
        assert a.is_zero == zero
        ra, rb = g.export_residues(a), o.export_residues(b)
        if zero:
            assert not ra.any()
        if not np.array_equal(ra, rb):
            bad = np.argwhere(ra != rb)
            raise AssertionError(f"output {r}: {len(bad)} of {ra.size} residues differ; first at "
                                 f"[batch, poly, limb, coeff] = {bad[0].tolist()}")
    del cg, co, og, oo
    _drop(g, o)


@pytest.mark.gpu
def test_lincomb_int_zero_inputs_and_columns(product_lib, oracle_lib, gpu_available):
    """A zero ciphertext contributes nothing and a column of zero weights is not read: the
    result is the combination of the others; with no contribution left, zero ciphertexts."""
    g, o = _pair(product_lib, oracle_lib, log_n=12, max_level=2, seed=5, special_primes=2)
    xs = _inputs(g.primes, 2, 2, 2, 2, seed=3, N=1 << 12)
    W = [[3, -4, 9], [0, 5, 0]]
    outs = []
    for e in (g, o):
        a, b = (e.import_residues(x) for x in xs)
        outs.append(e.lincomb_int([a, e.zeros(2, 2), b], W) + e.lincomb_int([e.zeros(2, 2), a], [[7, 0]]))
    for cg, co, zero in zip(outs[0], outs[1], (False, True, True)):
        assert cg.is_zero == co.is_zero == zero
        assert np.array_equal(g.export_residues(cg), o.export_residues(co))


@pytest.mark.gpu
def test_lincomb_int_refusals_take_no_pool_block(product_lib, gpu_available):
    g = Engine(_lib=product_lib, log_n=12, max_level=3, seed=5, special_primes=2)
    x = _pool(g.primes, 3, 4, 3, seed=1, n=1 << 12)
    a = g.import_residues(x[:, :2])
    low, three, small = g.import_residues(x[:, :2, :3]), g.import_residues(x), g.import_residues(x[:2, :2])
    g.synchronize()

    def call(cts, W):
        n, m = len(cts), len(W)
        arr = (c_ct_p * max(n, 1))(*[c._h for c in cts])
        wa = np.ascontiguousarray(np.array(W, dtype=np.int64).reshape(-1))
        wa = wa if wa.size else np.zeros(1, np.int64)
        outs = (c_ct_p * max(m, 1))()
        live = g.pool_stats()["live"]
        rc = g._lib.lincomb_int(g._h, arr, n, wa.ctypes.data_as(C.POINTER(C.c_int64)), m, outs)
        assert g.pool_stats()["live"] == live, "a refused call took a pool block"
        assert rc != 0 and not any(outs[i] for i in range(m))
        return rc

    assert call([a, low], [[1, 1]]) == ELEVEL
    assert call([a, small], [[1, 1]]) == EARG
    assert call([a, three], [[1, 1]]) == EDEGREE
    assert call([], [[]]) == EARG
    assert call([a] * 33, [[1] * 33]) == EARG
    assert call([a], [[1]] * 17) == EARG
    assert call([a], [[-(1 << 63)]]) == EARG
    # and the same inputs are fine within the limits: 32 inputs, 16 outputs
    assert len(g.lincomb_int([a] * 32, [[1] * 32])) == 1
    assert len(g.lincomb_int([a], [[r] for r in range(16)])) == 16


@pytest.mark.gpu
def test_times_is_one_launch(product_lib, gpu_available):
    """AESSlicedRound._times on the HIP engine: one lincomb_int launch, no chain of additions."""
    g = Engine(_lib=product_lib, log_n=12, max_level=3, seed=5, special_primes=2)
    R = AESSlicedRound.__new__(AESSlicedRound)
    R.e = g
    x = _pool(g.primes, 3, 1, 2, seed=2, n=1 << 12)
    ct = g.import_residues(x)
    out, prof = _profiled(g, lambda: R._times(ct, 37 << 7))
    assert prof.get("lincomb_int") == 1 and not prof.get("add"), prof
    assert np.array_equal(g.export_residues(out), lincomb_int_ref([x], [[37 << 7]], g.primes[:4])[0])

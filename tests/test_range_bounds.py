"""Residue parity at worst-case operands and across the 2^42 prime split.

The kernels in csrc/ lean on range bounds stated in comments (mul_m: a, b < q < 2^51; fred:
|x| < 2^53; k_dot: lazy sums folded every 16 pairs; k_rescale_spread: the centring test
v > (q_l >> 1)) and switch variant by prime size: kBigPrime = 2^42 picks the fold schedule of every
ntt256f.h pass, of the column base conversions and of k_moddown, and poly2_int picks one
of four kernel classes per limb from the weights' row sums against 2^52 / q and 2^51 / q.  The other
suites run uniformly random residues on chains whose primes all sit on one side of 2^42.  Here,
residue for residue against the CPU oracle (np.array_equal on export_residues, inputs through
import_residues, keys from identical seeds; no tolerance anywhere):

* Part A (N = 2^16): the seven-op key-switch sweep with its launch-profile check, the extreme
  ModUp source words and ntt_host on runs of q - 1 / 0, on chains whose primes straddle 2^42 inside
  digits and target tiles (S42), all lie just below 2^50 (S49) or are 30-bit under 50-bit special
  primes with a digit wider than K (S30);
* Part B (N = 2^12): the element-wise kernels on operands whose every word is chosen -- eighths of
  0, 1, q - 1, q - 2, (q - 1) / 2, (q + 1) / 2, 2^k - 1 and random values, rotated per operand so
  that (q - 1, q - 1), (q - 1, 0), (q - 1, 1) and ((q + 1) / 2, (q + 1) / 2) meet -- and full lazy
  sums of all-(q - 1) operands; the 3-polynomial tensor is also checked against Python integers;
* Part C: the rescale's centring boundary, the coefficient-domain top limb holding (q_l - 1) / 2
  and (q_l + 1) / 2, for rescale and for the level-down folded into a rescale;
* Part D: poly2_int's kernel classes (exact, lazy, folding, split) from poly2_plan(), the host's
  choice restated, with weights on either side of both thresholds and the launch count checked.
  The fold bound itself (|y'| near q / 2 with signs aligned to the weights) is not forced: y'
  carries a host-side constant H;
* Part E: the engine refuses a prime >= 2^50 that the oracle accepts.
"""
import ctypes as C
import math

import numpy as np
import pytest

from aes_xor_fhe._abi import Params
from aes_xor_fhe.fhe import Engine, widest_digits

from _ks_helpers import (N16, _check_construction, _check_path, _compare, _drop, _expect_out,  # noqa: E402
                         _extreme_ct, _keys, _ntt, _pair, _pool, _profiled, _sweep, ks_plan)
from _int_refs import tensor_ref as _tensor_ref  # noqa: E402  (the exact references live in one file)

BIG = 1 << 42  # kernels.h kBigPrime

# id -> scale_bits, K, A, L at log_n = 16 (base_bits = special_bits = 50), batch 1
CHAINS = {
    "S42": dict(scale_bits=42, K=4, A=4, L=8),  # both classes inside digits and target tiles
    "S49": dict(scale_bits=49, K=4, A=4, L=6),  # every prime big, as near 2^50 as the engine accepts
    "S30": dict(scale_bits=30, K=4, A=5, L=8),  # 30-bit sources under 50-bit targets, digit wider than K
}
# the classes of q_0..q_L ('B': >= 2^42), written from an oracle run; the CPU test pins them
S42_CLASSES = "BsBBsssBs"
SWEEP_LEVELS = {"l2": lambda L: 2, "below-top": lambda L: L - 1, "top": lambda L: L}
# Part B / C / D at N = 2^12: one chain with both classes, one with every prime near 2^49
PB = dict(log_n=12, max_level=6, special_primes=2, scale_bits=42, seed=21)
PB_CLASSES = "BBssBBs"
P49 = dict(log_n=12, max_level=4, special_primes=2, scale_bits=49, seed=22)
N12 = 1 << 12


def _kw(ident, seed=77):
    s = CHAINS[ident]
    return dict(log_n=16, max_level=s["L"], special_primes=s["K"], digit_primes=s["A"], scale_bits=s["scale_bits"],
                seed=seed)


def _chain(lib, log_n, max_level, special_primes, scale_bits):
    """The primes the library's chain call makes for these parameters (no engine)."""
    cp = Params(log_n, max_level, special_primes, scale_bits, 50, 50, 0, 0, 0, None)
    primes = (C.c_uint64 * (max_level + 1 + special_primes))()
    scales = (C.c_double * (max_level + 1))()
    lib.check(lib.chain(C.byref(cp), primes, scales))
    return [int(q) for q in primes]


def _classes(primes):
    return "".join("B" if q >= BIG else "s" for q in primes)


def _same(g, o, cg, co, what):
    """Two results of any polynomial count: same shape, same residues."""
    assert (cg.level, cg.batch, cg.npoly, cg.is_zero) == (co.level, co.batch, co.npoly, co.is_zero), \
        f"{what}: {cg!r} vs {co!r}"
    a, b = g.export_residues(cg), o.export_residues(co)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} residues differ; first at "
                             f"[batch, poly, limb, coeff] = {bad[0].tolist()}, {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}")
    return a


# ------------------------------------------------------------------------------------------------
# Part A (CPU): the facts the chain table relies on
def test_chain_classes_on_the_oracle(oracle_lib):
    """A change to make_chain cannot quietly remove the coverage: S42 has both classes among
    q_1..q_L and inside a digit, S49 is all big and below 2^50, S30 all small; ks_plan agrees with
    each chain's (K, A)."""
    pr = {c: _chain(oracle_lib, 16, s["L"], s["K"], s["scale_bits"]) for c, s in CHAINS.items()}
    s42, L = pr["S42"], CHAINS["S42"]["L"]
    assert _classes(s42[:L + 1]) == S42_CLASSES
    assert {"B", "s"} == set(_classes(s42[1:L + 1]))
    digits = [_classes(s42[lo:min(lo + 4, L + 1)]) for lo in range(0, L + 1, 4)]
    assert digits == ["BsBB", "sssB", "s"] and sum(len(set(d)) == 2 for d in digits) >= 1
    # neighbouring targets of one k_bconv_cols tile of four (ModDown targets q_0..) differ in class
    assert any(len(set(_classes(s42[t:t + 4]))) == 2 for t in range(0, L + 1, 4))
    assert all(BIG <= q < 1 << 50 for q in pr["S49"])
    assert max(pr["S49"][1:CHAINS["S49"]["L"] + 1]) > 1 << 49  # chain primes on both sides of 2^49
    assert all(q < BIG for q in pr["S30"][1:CHAINS["S30"]["L"] + 1]) and all(q >= BIG for q in pr["S30"][9:])
    assert all(q < 1 << 32 for q in pr["S30"][1:9])  # 4-byte source words
    for c, s in CHAINS.items():
        want = 4 if c != "S30" else 5
        assert widest_digits(16, s["L"], s["K"], s["scale_bits"], lib=oracle_lib) == want
        assert s["A"] == want and (c != "S30" or s["A"] > s["K"])
    assert ks_plan(4, 4, 8, 0, "relinearize")["digits"] == [4, 4, 1] and ks_plan(4, 4, 8, 0, "rotate")["spread"] == 1
    assert ks_plan(4, 4, 6, 1, "multiply")["digits"] == [4, 3] and ks_plan(4, 4, 6, 1, "multiply")["vslot"] == 5
    p = ks_plan(4, 5, 8, 2, "poly2_int")
    assert p["digits"] == [5, 4] and p["modup_nstep"] == [1, 2] and p["modup_nt"] == [8, 9] and p["vslot"] == 6
    assert [[f(s["L"]) for f in SWEEP_LEVELS.values()] for s in CHAINS.values()] == [[2, 7, 8], [2, 5, 6], [2, 7, 8]]
    # the N = 2^12 chains of Parts B-D
    pb = _chain(oracle_lib, 12, PB["max_level"], PB["special_primes"], PB["scale_bits"])
    assert _classes(pb[:PB["max_level"] + 1]) == PB_CLASSES
    p49 = _chain(oracle_lib, 12, P49["max_level"], P49["special_primes"], P49["scale_bits"])
    assert all(1 << 48 < q < 1 << 50 for q in p49)


# ------------------------------------------------------------------------------------------------
# Part A (GPU)
@pytest.fixture(scope="module")
def chain_pair(request, product_lib, oracle_lib, gpu_available):
    """One 2^16 engine pair with its keys per chain (indirect parameter: the chain's id), released
    with pool_trim before the next one.  Every test lists the chains in CHAINS' order in a
    parametrize of its own, so that pytest groups the module's tests by chain."""
    ident = request.param
    s = CHAINS[ident]
    g, o = _pair(product_lib, oracle_lib, **_kw(ident))
    assert g.digit_primes == s["A"] and g.special_prime_count == s["K"]
    st = dict(ident=ident, g=g, o=o, kg=_keys(g), ko=_keys(o), pool=_pool(g.primes, s["L"], 1, 6, seed=4200 + s["L"]),
              **s)
    yield st
    st.clear()
    _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("chain_pair", list(CHAINS), indirect=True)
@pytest.mark.parametrize("level", list(SWEEP_LEVELS))
def test_prime_class_sweep_bit_exact(chain_pair, level):
    st = chain_pair
    l = SWEEP_LEVELS[level](st["L"])
    _sweep(st["g"], st["o"], st["kg"], st["ko"], st["ident"], st["K"], st["A"], 1, [l], st["pool"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("chain_pair", ["S42", "S49"], indirect=True)
def test_prime_class_extreme_source_words_bit_exact(chain_pair):
    st = chain_pair
    g, o, K, A, l = st["g"], st["o"], st["K"], st["A"], st["L"]
    arr, want = _extreme_ct(o, A, l, seed=540 + l)
    co = _check_construction(o, arr, want)
    what = f"engine {st['ident']} (extreme source words), op relinearize, level {l}, batch 1"
    og, prof = _profiled(g, lambda: [g.relinearize(g.import_residues(arr), st["kg"]["rlk"])])
    _check_path(prof, K, A, l, "relinearize", what)
    _compare(g, o, og, [o.relinearize(co, st["ko"]["rlk"])], _expect_out("relinearize", l, 1), what)


def _ntt_inputs(primes, n, seed):
    """Two inputs per prime: the `extreme` pattern of test_ntt_bit_exact (a run of q - 1, then
    every third coefficient 0 among random ones), and 0 / q - 1 alternating."""
    rng = np.random.default_rng(seed)
    ext = np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in primes])
    alt = np.zeros_like(ext)
    for r, q in enumerate(primes):
        ext[r, :n // 2] = q - 1
        ext[r, n // 2::3] = 0
        alt[r, 1::2] = q - 1
    return dict(extreme=ext, alternating=alt)


def _ntt_all(eng, limbs, inverse):
    buf = limbs.copy()
    pids = np.arange(len(limbs), dtype=np.int32)
    eng._check(eng._lib.ntt_host(eng._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), len(limbs),
                                 pids.ctypes.data_as(C.POINTER(C.c_int32)), inverse))
    return buf


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("chain_pair", list(CHAINS), indirect=True)
def test_prime_class_ntt_bit_exact(chain_pair):
    """ntt_host forward and inverse on the chain's full prime list (chain and special primes)."""
    g, o = chain_pair["g"], chain_pair["o"]
    for name, limbs in _ntt_inputs(g.primes, N16, seed=16).items():
        for inverse in (0, 1):
            a, b = _ntt_all(g, limbs, inverse), _ntt_all(o, limbs, inverse)
            bad = np.argwhere(a != b)
            assert not len(bad), (f"{chain_pair['ident']} ntt_host {name} inverse={inverse}: {len(bad)} differ, "
                                  f"first at [prime, coeff] = {bad[0].tolist()}")


# ------------------------------------------------------------------------------------------------
# Part B: worst-case operands straight into the element-wise kernels
def _edge_values(q):
    return [0, 1, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, (1 << (q.bit_length() - 1)) - 1]


def _edge_limb(q, n, rot, rng):
    """n words in contiguous eighths: eighth e holds pattern (e + rot) % 8 of 0, 1, q - 1, q - 2,
    (q - 1) / 2, (q + 1) / 2, the largest 2^k - 1 below q, uniformly random values."""
    e = n // 8
    vals = _edge_values(q)
    out = np.empty(n, dtype=np.uint64)
    for k in range(8):
        p = (k + rot) % 8
        out[k * e:(k + 1) * e] = vals[p] if p < 7 else rng.integers(0, q, e, dtype=np.uint64)
    return out


def _edge_pool(primes, l, rots, seed, n=N12):
    """(B, npoly, l + 1, n) residues; rots[b][p]: the rotation of the eighths of (batch b, poly p)."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(rots), len(rots[0]), l + 1, n), dtype=np.uint64)
    for b, row in enumerate(rots):
        for p, rot in enumerate(row):
            for i in range(l + 1):
                out[b, p, i] = _edge_limb(primes[i], n, rot, rng)
    return out


# rotations of (batch, poly) of the three operands: a0 b0 meet at 0 (batch 0: (q - 1, q - 1),
# ((q + 1) / 2, (q + 1) / 2)) and at 7 (batch 1: (q - 1, 1)), a0 b1 at 6 (batch 0: (q - 1, 0))
ROT_A, ROT_B, ROT_C = [[0, 3], [0, 5]], [[0, 6], [7, 2]], [[7, 1], [6, 0]]


def _const_pool(primes, l, B, npoly, value, n=N12):
    """Every word value(q): all-(q - 1) is _const_pool(.., lambda q: q - 1)."""
    out = np.empty((B, npoly, l + 1, n), dtype=np.uint64)
    for i in range(l + 1):
        out[:, :, i] = value(primes[i])
    return out


def _tensor(e, x, y):
    """aesfhe_tensor of two imported arrays (the operands stay referenced across the call)."""
    a, b = e.import_residues(x), e.import_residues(y)
    return e._call_ct(e._lib.tensor, a._h, b._h)


def _mul_const(e, x, c):
    a = e.import_residues(x)
    return e._call_ct(e._lib.mul_const, a._h, complex(c).real, complex(c).imag)


def _pb_operands(primes, l):
    return (_edge_pool(primes, l, ROT_A, 31), _edge_pool(primes, l, ROT_B, 32), _edge_pool(primes, l, ROT_C, 33))


def test_edge_pool_meetings_and_tensor_reference_on_the_oracle(oracle_lib):
    """The operand pool holds the pairs it is there for, and the Python-integer tensor reference
    equals the oracle's aesfhe_tensor on it (the oracle is then not the only witness on the GPU)."""
    o = Engine(_lib=oracle_lib, **PB)
    l = o.max_level
    assert _classes(o.primes[:l + 1]) == PB_CLASSES
    a, b, c = _pb_operands(o.primes, l)
    assert a.shape == b.shape == c.shape == (2, 2, l + 1, N12)
    for i, q in enumerate(o.primes[:l + 1]):
        assert int(a[:, :, i].max()) == q - 1 and int(b[:, :, i].max()) == q - 1 and int(c[:, :, i].max()) == q - 1
        both = lambda x, u, y, v: bool(((x == u) & (y == v)).any())  # noqa: E731
        assert both(a[0, 0, i], q - 1, b[0, 0, i], q - 1)
        assert both(a[0, 0, i], (q + 1) // 2, b[0, 0, i], (q + 1) // 2)
        assert both(a[0, 0, i], q - 1, b[0, 1, i], 0)
        assert both(a[1, 0, i], q - 1, b[1, 0, i], 1)
        for v in _edge_values(q):
            assert (a[0, 0, i] == v).sum() >= N12 // 8
    t = _tensor(o, a, b)
    assert (t.level, t.batch, t.npoly) == (l, 2, 3)
    assert np.array_equal(o.export_residues(t), _tensor_ref(a, b, o.primes))
    ones = _const_pool(o.primes, l, 2, 2, lambda q: q - 1)
    assert all(int(ones[:, :, i].min()) == q - 1 for i, q in enumerate(o.primes[:l + 1]))


@pytest.fixture(scope="module")
def pb_pair(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **PB)
    l = g.max_level
    assert _classes(g.primes[:l + 1]) == PB_CLASSES and {"B", "s"} == set(PB_CLASSES[1:])
    a, b, c = _pb_operands(g.primes, l)
    st = dict(g=g, o=o, l=l, a=a, b=b, c=c, top=_const_pool(g.primes, l, 2, 2, lambda q: q - 1),
              one=_const_pool(g.primes, l, 2, 2, lambda q: 1))
    for eng, k in ((g, "kg"), (o, "ko")):
        st[k] = eng.create_relinearization_key(eng.create_secret_key(9))
    yield st
    st.clear()
    _drop(g, o)


def _both(st, fn, what):
    """fn(engine, rlk) on both engines: the results are the same."""
    rg, ro = fn(st["g"], st["kg"]), fn(st["o"], st["ko"])
    if isinstance(rg, (list, tuple)):
        assert len(rg) == len(ro)
        return [_same(st["g"], st["o"], x, y, f"{what} out {i}") for i, (x, y) in enumerate(zip(rg, ro))]
    return _same(st["g"], st["o"], rg, ro, what)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_elementwise_edge_operands_bit_exact(pb_pair):
    st = pb_pair
    a, b, c = st["a"], st["b"], st["c"]
    imp = lambda e, x: e.import_residues(x)  # noqa: E731
    _both(st, lambda e, k: e.add(imp(e, a), imp(e, b)), "add")
    _both(st, lambda e, k: e.subtract(imp(e, a), imp(e, b)), "subtract")
    _both(st, lambda e, k: e.subtract(imp(e, b), imp(e, a)), "subtract (swapped)")
    _both(st, lambda e, k: e.negate(imp(e, a)), "negate")
    _both(st, lambda e, k: e.add(imp(e, st["top"]), imp(e, st["top"])), "add of all-(q-1)")
    _both(st, lambda e, k: e.multiply_fma(imp(e, a), imp(e, b), k, alpha=3, c=imp(e, c), gamma=0.5, beta=0.25),
          "multiply_fma")
    _both(st, lambda e, k: e.multiply_fma(imp(e, st["top"]), imp(e, st["top"]), k, alpha=-7, c=imp(e, st["top"]),
                                          gamma=-1.0, beta=-0.5), "multiply_fma of all-(q-1)")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_tensor_edge_operands_bit_exact_and_python_integers(pb_pair):
    """multiply without a key: the 3-polynomial k_tensor output, rescaled; the tensor itself is
    also compared with Python integers."""
    st = pb_pair
    g = st["g"]
    for name, x, y in (("a x b", st["a"], st["b"]), ("b x c", st["b"], st["c"]), ("top x top", st["top"], st["top"]),
                       ("top x a", st["top"], st["a"])):
        got = _both(st, lambda e, k: _tensor(e, x, y), f"tensor {name}")
        ref = _tensor_ref(x, y, g.primes)
        bad = np.argwhere(got != ref)
        assert not len(bad), f"tensor {name} vs Python integers: {len(bad)} differ, first at {bad[0].tolist()}"
        r = _both(st, lambda e, k: e.multiply(e.import_residues(x), e.import_residues(y)), f"multiply {name} (no key)")
        assert r.shape == (2, 3, st["l"], N12)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_and_constant_edge_operands_bit_exact(pb_pair):
    st = pb_pair
    a, top = st["a"], st["top"]
    vec = np.exp(2j * np.pi * np.arange(N12 // 2) / 7.0) * 3.25
    for name, x in (("a", a), ("top", top)):
        imp = lambda e: e.import_residues(x)  # noqa: E731
        for cst in (3.0, -2.5 + 1.5j):
            _both(st, lambda e, k: e.multiply(imp(e), cst), f"multiply {name} by {cst} (deferred)")
            _both(st, lambda e, k: _mul_const(e, x, cst), f"mul_const {name} by {cst}")
            _both(st, lambda e, k: e.add(imp(e), cst), f"add_const {name} {cst}")
        _both(st, lambda e, k: e.multiply(imp(e), e.encode(vec)), f"multiply {name} by a plaintext")
        _both(st, lambda e, k: e.add(imp(e), e.encode(vec)), f"add {name} and a plaintext")
        _both(st, lambda e, k: e.subtract(imp(e), vec), f"subtract a plaintext from {name}")


LINCOMB_N = (1, 8, 9, 63, 64)
DOT_N = (1, 15, 16, 17, 32, 33)


def _coeffs(n, kind, scale, seed):
    """unit: every constant rounds to 1, so every term of all-(q - 1) inputs is q - 1 and the lazy
    sum is n (q - 1), its largest; complex: seeded complex coefficients of magnitude up to 4."""
    if kind == "unit":
        return np.full(n, 1.0 / scale, dtype=np.complex128)
    rng = np.random.default_rng(seed)
    return rng.uniform(-4, 4, n) + 1j * rng.uniform(-4, 4, n)


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", LINCOMB_N)
def test_lincomb_full_lazy_sums_bit_exact(pb_pair, n):
    st = pb_pair
    scale = st["o"]._lib.engine_mul_scale(st["o"]._h, st["l"])
    assert scale == st["g"]._lib.engine_mul_scale(st["g"]._h, st["l"]) and round(1.0 / scale * scale) == 1
    for kind in ("unit", "complex"):
        co = _coeffs(n, kind, scale, 100 + n)

        def run(e, k, last="top"):
            top = e.import_residues(st["top"])
            return e.lincomb([top] * (n - 1) + [e.import_residues(st[last])], co)
        _both(st, run, f"lincomb n={n} {kind}")
        # -n is the same small integer in every limb and rescales to zero: with the edge pool as
        # the last input the sum still reaches n (q - 1) (its eighth of q - 1) and the result is not
        _both(st, lambda e, k: run(e, k, "a"), f"lincomb n={n} {kind}, last input the edge pool")
    if n == 64:  # distinct inputs as well: the edge pool under the all-(q-1) ciphertexts
        def run(e, k):
            xs = [e.import_residues(st[x]) for x in ("a", "b", "c", "top")]
            return e.lincomb([xs[i % 4] for i in range(n)], _coeffs(n, "complex", scale, 7))
        _both(st, run, "lincomb n=64 mixed inputs")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_lincomb_at_the_abi_limit_bit_exact(pb_pair):
    """n = 4096, the most aesfhe_lincomb admits (engine.hip), of all-(q - 1) inputs with unit
    constants: k_lincomb's u64 lazy sum reaches 4096 (q - 1), 2^62 on the 50-bit q_0 -- the largest
    value its single red_m (x < 2^63) ever sees."""
    st = pb_pair
    n = 4096
    scale = st["o"]._lib.engine_mul_scale(st["o"]._h, st["l"])

    def run(e, k):  # the last input the edge pool: -4096 in every limb would rescale to zero
        top = e.import_residues(st["top"])
        return e.lincomb([top] * (n - 1) + [e.import_residues(st["a"])], _coeffs(n, "unit", scale, 0))
    got = _both(st, run, f"lincomb n={n} unit")
    assert got.any()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_lincomb_many_bit_exact(pb_pair):
    st = pb_pair
    n, m = 16, 3
    scale = st["o"]._lib.engine_mul_scale(st["o"]._h, st["l"])
    M = np.stack([_coeffs(n, "unit", scale, 0), _coeffs(n, "complex", scale, 41), _coeffs(n, "complex", scale, 42).real])

    def run(e, k):
        top, a, b = (e.import_residues(st[x]) for x in ("top", "a", "b"))
        return e.lincomb_many([top] * n, M) + e.lincomb_many([top, a, b, top] * 4, M)
    outs = _both(st, run, f"lincomb_many n={n} m={m}")
    assert len(outs) == 2 * m


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", DOT_N)
def test_dot_full_lazy_sums_bit_exact(pb_pair, n):
    """n pairs of all-(q - 1) operands ((q - 1)^2 = 1 mod q: the smallest products), and n pairs of
    all-(q - 1) with all-1 operands (every product q - 1: the lazy sums d0, d2 = n (q - 1) and
    d1 = 2 n (q - 1) that the fold at (i & 15) == 15 is there for)."""
    st = pb_pair
    for name, y in (("top . top", "top"), ("top . one", "one"), ("top . b", "b")):
        def run(e, k, fma=False):
            p, r = e.import_residues(st["top"]), e.import_residues(st[y])
            if fma:
                return e.dot_fma([p] * n, [r] * n, k, addends=[(e.import_residues(st["c"]), -3.0), (p, 1.0)], beta=0.75)
            return e.dot([p] * n, [r] * n, k)
        _both(st, run, f"dot n={n} {name}")
        _both(st, lambda e, k: run(e, k, True), f"dot_fma n={n} {name}")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_dot_fma_without_products_and_the_limits_on_n(pb_pair):
    """k_dot_fma with no pair left (the only pair has a zero operand) plus addends; and the limits
    on n (engine.hip: lincomb 1..4096, dot / dot_fma n >= 1, poly2_int nx, ny <= 16): one past each
    raises in both engines instead of running."""
    st = pb_pair

    def run(e, k):
        z, p = e.zeros(2, st["l"]), e.import_residues(st["top"])
        return e.dot_fma([z], [p], k, addends=[(p, 1.0), (e.import_residues(st["a"]), -2.0)], beta=-0.25)
    _both(st, run, "dot_fma with a zero pair + addends")
    for e, k in ((st["g"], st["kg"]), (st["o"], st["ko"])):
        p = e.import_residues(st["top"])
        with pytest.raises(RuntimeError, match="empty linear combination"):
            e.lincomb([], [])
        with pytest.raises(RuntimeError, match="linear combination too long"):
            e.lincomb([p] * 4097, np.ones(4097))
        with pytest.raises(RuntimeError, match="empty dot product"):
            e.dot([], [], k)
        with pytest.raises(RuntimeError, match="empty dot product"):
            e.dot_fma([], [], k, addends=[(p, 1.0)])
        with pytest.raises(RuntimeError, match="nx, ny <= 16"):
            e.poly2_int([p] * 16, [p], np.ones((1, 17, 2), dtype=np.int64), 64, k)


# ------------------------------------------------------------------------------------------------
# Part C: the rescale's centring boundary
def _centre_pattern(q, n, rng):
    """The coefficient-domain top limb: eighths of 0, 1, (q - 1) / 2, (q + 1) / 2, q - 1, q - 2 and
    two of random values.  (q - 1) / 2 = q >> 1 is the largest word not centred, (q + 1) / 2 the
    smallest that is."""
    e = n // 8
    v = np.empty(n, dtype=np.uint64)
    for k, x in enumerate((0, 1, (q - 1) // 2, (q + 1) // 2, q - 1, q - 2)):
        v[k * e:(k + 1) * e] = x
    v[6 * e:] = rng.integers(0, q, 2 * e, dtype=np.uint64)
    return v


def _level_down_const(o, l):
    """engine.hip level_down_const(from = l, to = l - 1): the constant folded into the rescale."""
    return int(math.floor(o.scales[l - 1] * float(o.primes[l]) / o.scales[l] + 0.5))


def _centre_ct(o, l, npoly, B, seed, folded):
    """(B, npoly, l + 1, n) random residues whose limb l is, in coefficient form, the pattern
    (folded: the pattern times C^{-1}, so that C x, what the folded level-down centres, is the
    pattern).  Returns the array and {(b, p): pattern}."""
    n = 1 << o.log_coeff_count
    q = o.primes[l]
    rng = np.random.default_rng(seed)
    arr = _pool(o.primes, l, B, npoly, seed + 1, n=n)
    cinv = pow(_level_down_const(o, l) % q, -1, q) if folded else 1
    want = {}
    for b in range(B):
        for p in range(npoly):
            v = _centre_pattern(q, n, rng)
            x = np.array((v.astype(object) * cinv) % q, dtype=np.uint64)
            arr[b, p, l] = _ntt(o, x, l, 0)
            want[b, p] = v
    return arr, want


def _check_centre(o, arr, want, l, folded):
    """The oracle's inverse NTT of the imported top limb (times C when folded) is the pattern."""
    ct = o.import_residues(arr)
    back = o.export_residues(ct)
    assert np.array_equal(back, arr)
    q = o.primes[l]
    c = _level_down_const(o, l) % q if folded else 1
    for (b, p), v in want.items():
        x = _ntt(o, back[b, p, l], l, 1)
        assert np.array_equal(np.array((x.astype(object) * c) % q, dtype=np.uint64), v), (b, p)
        half = q >> 1
        assert (v == half).sum() >= len(v) // 8 and (v == half + 1).sum() >= len(v) // 8
    return ct


def _centre_cases(g, o, l, B, what):
    """rescale and the level-down by one level (rescale_view with the constant folded in), on 2-
    and 3-polynomial ciphertexts (the fused spread of the column pass at N = 2^16 for 2
    polynomials, k_rescale_spread otherwise)."""
    for npoly in (2, 3):
        for folded in (False, True):
            arr, want = _centre_ct(o, l, npoly, B, 900 + 10 * l + npoly, folded)
            co = _check_centre(o, arr, want, l, folded)
            cg = g.import_residues(arr)
            name = f"{what} level {l}, {npoly} polynomials, " + ("level_down" if folded else "rescale")
            if folded:
                _same(g, o, g.level_down(cg, l - 1), o.level_down(co, l - 1), name)
            else:
                _same(g, o, g.rescale(cg), o.rescale(co), name)


def test_centre_construction_on_the_oracle(oracle_lib):
    o = Engine(_lib=oracle_lib, **PB)
    for l in (o.max_level, o.max_level - 1):
        for folded in (False, True):
            arr, want = _centre_ct(o, l, 2, 2, 900 + l, folded)
            ct = _check_centre(o, arr, want, l, folded)
            out = o.level_down(ct, l - 1) if folded else o.rescale(ct)
            assert (out.level, out.batch, out.npoly) == (l - 1, 2, 2)
    assert PB_CLASSES[o.max_level] != PB_CLASSES[o.max_level - 1]
    assert S42_CLASSES[8] != S42_CLASSES[7]


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_rescale_centring_boundary_bit_exact(pb_pair):
    st = pb_pair
    for l in (st["l"], st["l"] - 1):  # top prime small, top prime big
        _centre_cases(st["g"], st["o"], l, 2, "N = 2^12")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("chain_pair", ["S42"], indirect=True)
@pytest.mark.parametrize("l", [8, 7])
def test_rescale_centring_boundary_n16_bit_exact(chain_pair, l):
    assert S42_CLASSES[l] == ("s" if l == 8 else "B")
    _centre_cases(chain_pair["g"], chain_pair["o"], l, 1, "S42")


# ------------------------------------------------------------------------------------------------
# Part D: poly2_int's kernel classes
def poly2_plan(primes, W, n):
    """The launches of aesfhe_poly2_int's inner-sum kernels (engine.hip poly2_int_impl, the wfac /
    wfac_u block) from the level's primes q_0..q_l, the integer weights W (m, nx, ny) and N alone:
    [(t0, la, lb, class)], one launch per entry, for limbs la..lb-1 of the outputs from live index
    t0.  Classes: 'split' (k_poly2_int_split: big limbs below 2^51 in the S-box shape), 'folding'
    (the folding kernel: big limbs otherwise), 'lazy' (k_poly2_int_s with y' unreduced), 'exact'.
    A run ends where is_big or lazy_ok changes, so neighbouring runs may share a class in the
    generic shape, which has no lazy kernel."""
    W = np.asarray(W)
    m, nx, ny = W.shape
    wfac = 1.0
    for t in range(m):
        for i in range(nx):
            f = 0.0
            for j in range(ny):
                a = float(abs(int(W[t, i, j])))
                f += a if j == 0 else 0.5 * a + 1e-3 * a
            assert np.abs(W[t, i]).sum() <= 512
            wfac = max(wfac, f)
    live = [t for t in range(m) if W[t].any()]
    wfac_u = max([1.0] + [float(np.abs(W[t, i]).sum()) for t in live for i in range(nx)])
    is_big = lambda q: wfac * q >= 2.0 ** 52 * 0.999 or (wfac + 3.0 * nx) * q >= 2.0 ** 53 * 0.999  # noqa: E731
    lazy_ok = lambda q: wfac_u * q < 2.0 ** 51 and (wfac_u + 3.0 * nx) * q < 2.0 ** 52  # noqa: E731
    ml, nl, t0, out = len(live), len(primes), 0, []
    while t0 < ml:
        sbox = ny == 16 and ml - t0 >= 8 and (n // 256) % 8 == 0
        la = 0
        while la < nl:
            big = is_big(float(primes[la]))
            lz = not big and lazy_ok(float(primes[la]))
            lb = la + 1
            while lb < nl and is_big(float(primes[lb])) == big and (big or lazy_ok(float(primes[lb])) == lz):
                lb += 1
            split = big and all(q < 1 << 51 for q in primes[la:lb])
            if sbox:
                cls = "split" if split else "folding" if big else "lazy" if lz else "exact"
            else:
                cls = "folding" if big else "exact"
            out.append((t0, la, lb, cls))
            la = lb
        t0 += 8 if sbox else 4
    return out


def _sbox_weights(row_sum, seed):
    """(8, 16, 16) weights in -3..3 with one row (output 5, x power 2) of |w| summing to row_sum."""
    rng = np.random.default_rng(seed)
    W = rng.integers(-3, 4, (8, 16, 16))
    row = np.full(16, row_sum // 16) + (np.arange(16) < row_sum % 16)
    W[5, 2] = row * np.where(np.arange(16) % 2, -1, 1)
    assert np.abs(W).sum(axis=2).max() == row_sum == np.abs(W[5, 2]).sum()
    return W


# generic shape (nx = 2, ny = 3; W[1] = 0 is a zero output): wfac = |w_0| + 0.501 sum_{j>0} |w_j|
W_G_LOW = np.array([[[0, 1, 0], [1, -1, 0]], [[0, 0, 0], [0, 0, 0]], [[1, 0, -1], [0, 1, 1]]])  # wfac 1.501
W_G_753 = np.array([[[0, 3, 0], [0, 8, -7]], [[0, 0, 0], [0, 0, 0]], [[1, -4, 2], [2, -1, 1]]])  # wfac 7.515
W_G_800 = np.array([[[0, 3, 0], [-8, 0, 0]], [[0, 0, 0], [0, 0, 0]], [[1, -4, 2], [2, -1, 1]]])  # wfac 8
W_G_511 = np.array([[[0, 3, 0], [171, -170, 170]], [[0, 0, 0], [0, 0, 0]], [[1, -4, 2], [2, -1, 1]]])
W_G_512 = np.array([[[0, 3, 0], [172, -170, 170]], [[0, 0, 0], [0, 0, 0]], [[1, -4, 2], [2, -1, 1]]])


def test_poly2_plan_hand_values(oracle_lib):
    """poly2_plan against values written by hand from engine.hip: the bench chain (q_0 50-bit,
    q_i near 2^40) with the AES S-box weights, S42 and the two N = 2^12 chains."""
    from aes_xor_fhe.aes_round_bits import walsh_sbox
    W = np.rint(walsh_sbox() * 64).astype(np.int64)
    assert W.shape == (8, 16, 16) and np.abs(W).sum(axis=2).max() == 76
    bench = _chain(oracle_lib, 16, 30, 10, 40)
    # wfac = 42.07, wfac_u = 76: q_0 is big ((42 + 48) 2^50 > 2^53) and below 2^51: split; 76 q and
    # (76 + 48) q stay below 2^51 / 2^52 for q near 2^40 or 2^42: lazy
    assert poly2_plan(bench[:27], W, N16) == [(0, 0, 1, "split"), (0, 1, 27, "lazy")]
    s42 = _chain(oracle_lib, 16, 8, 4, 42)
    assert poly2_plan(s42[:9], W, N16) == [(0, 0, 1, "split"), (0, 1, 9, "lazy")]
    # a row sum of 512: 512 q < 2^51 only for q < 2^42 -- the small limbs stay lazy, the big chain
    # limbs (B s B B s s s B s) take the exact kernel; 511: every chain limb lazy
    assert poly2_plan(s42[:9], _sbox_weights(512, 1), N16) == [
        (0, 0, 1, "split"), (0, 1, 2, "lazy"), (0, 2, 4, "exact"), (0, 4, 7, "lazy"), (0, 7, 8, "exact"),
        (0, 8, 9, "lazy")]
    assert poly2_plan(s42[:9], _sbox_weights(511, 1), N16) == [(0, 0, 1, "split"), (0, 1, 9, "lazy")]
    pb = _chain(oracle_lib, 12, 6, 2, 42)  # B B s s B B s
    assert poly2_plan(pb[:7], _sbox_weights(512, 1), N12) == [
        (0, 0, 1, "split"), (0, 1, 2, "exact"), (0, 2, 4, "lazy"), (0, 4, 6, "exact"), (0, 6, 7, "lazy")]
    assert poly2_plan(pb[:7], _sbox_weights(511, 1), N12) == [(0, 0, 1, "split"), (0, 1, 7, "lazy")]
    # below N = 2^11 the S-box shape takes the generic kernels, 4 outputs per launch
    assert poly2_plan(pb[:7], _sbox_weights(511, 1), 1 << 10) == [
        (t0, la, lb, c) for t0 in (0, 4) for la, lb, c in ((0, 1, "folding"), (1, 7, "exact"))]
    # the generic shape: q_0 exact for wfac 1.501 ((1.501 + 6) 2^50 < 2^53) but not lazy_ok, unlike
    # the chain limbs -- two runs of the same kernel; folding from wfac 3.996 on
    assert poly2_plan(pb[:7], W_G_LOW, N12) == [(0, 0, 1, "exact"), (0, 1, 7, "exact")]
    assert poly2_plan(pb[:7], W_G_753, N12) == [(0, 0, 1, "folding"), (0, 1, 7, "exact")]
    assert poly2_plan(pb[:7], W_G_511, N12) == [(0, 0, 1, "folding"), (0, 1, 7, "exact")]
    assert poly2_plan(pb[:7], W_G_512, N12) == [(0, 0, 1, "folding"), (0, 1, 2, "exact"), (0, 2, 4, "exact"),
                                                (0, 4, 6, "exact"), (0, 6, 7, "exact")]
    # every prime near 2^49: 2^52 / q is 8 -- wfac 7.515 leaves the chain limbs exact, 8 folds them;
    # in the S-box shape (wfac + 48) q > 2^53 whatever the weights: one split launch
    p49 = _chain(oracle_lib, 12, 4, 2, 49)
    assert poly2_plan(p49[:5], W_G_753, N12) == [(0, 0, 1, "folding"), (0, 1, 5, "exact")]
    assert poly2_plan(p49[:5], W_G_800, N12) == [(0, 0, 5, "folding")]
    assert poly2_plan(p49[:5], _sbox_weights(48, 1), N12) == [(0, 0, 5, "split")]
    classes = {c for pr, w in ((pb[:7], _sbox_weights(512, 1)), (pb[:7], W_G_753), (p49[:5], W_G_800))
               for _, _, _, c in poly2_plan(pr, w, N12)}
    assert classes == {"exact", "lazy", "folding", "split"}


POLY2_CASES = {
    # id: (chain, weights) -- what poly2_plan says of it is asserted in test_poly2_plan_hand_values
    "pb-sbox-512": ("pb", lambda: _sbox_weights(512, 1)),  # split, exact and lazy; 2^51 / q from above
    "pb-sbox-511": ("pb", lambda: _sbox_weights(511, 1)),  # 2^51 / q from below: every chain limb lazy
    "pb-generic-low": ("pb", lambda: W_G_LOW),  # q_0 exact
    "pb-generic-753": ("pb", lambda: W_G_753),  # q_0 folding
    "pb-generic-511": ("pb", lambda: W_G_511),
    "pb-generic-512": ("pb", lambda: W_G_512),
    "p49-generic-753": ("p49", lambda: W_G_753),  # 2^52 / q from below: chain limbs exact
    "p49-generic-800": ("p49", lambda: W_G_800),  # from above: chain limbs folding
    "p49-sbox": ("p49", lambda: _sbox_weights(48, 1)),  # split on chain limbs
}


@pytest.fixture(scope="module")
def p49_pair(product_lib, oracle_lib, gpu_available):
    g, o = _pair(product_lib, oracle_lib, **P49)
    st = dict(g=g, o=o, l=g.max_level)
    for eng, k in ((g, "kg"), (o, "ko")):
        st[k] = eng.create_relinearization_key(eng.create_secret_key(9))
    yield st
    st.clear()
    _drop(g, o)


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", list(POLY2_CASES))
def test_poly2_int_kernel_classes_bit_exact(pb_pair, p49_pair, case):
    chain, wf = POLY2_CASES[case]
    st = pb_pair if chain == "pb" else p49_pair
    g, o, l = st["g"], st["o"], st["l"]
    W = wf()
    m, nx, ny = W.shape
    plan = poly2_plan(g.primes[:l + 1], W, N12)
    # basis element i: the edge pool with its eighths rotated by i (batch 1: by i + 3), batch 2
    xs = [_edge_pool(g.primes, l, [[i, i + 5], [i + 3, i + 6]], 600 + i) for i in range(nx - 1)]
    ys = [_edge_pool(g.primes, l, [[i + 1, i + 2], [i + 7, i + 4]], 700 + i) for i in range(ny - 1)]

    def run(e, k):
        return e.poly2_int([e.import_residues(x) for x in xs], [e.import_residues(y) for y in ys], W, 64, k)
    og, prof = _profiled(g, lambda: run(g, st["kg"]), field=3)  # kernel dispatches per label
    assert prof.get("poly2_int", 0) == len(plan), f"{case}: {prof.get('poly2_int')} launches, plan {plan}"
    oo = run(o, st["ko"])
    expect = [(l - 2, 2, not W[t].any()) for t in range(m)]
    _compare(g, o, og, oo, expect, f"poly2_int {case}")


# ------------------------------------------------------------------------------------------------
# Part E: the 2^50 limit
@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_engine_refuses_primes_above_2_50(product_lib, oracle_lib, gpu_available):
    kw = dict(log_n=16, special_primes=4, max_level=6)
    primes = _chain(product_lib, 16, 6, 4, 50)
    assert primes == _chain(oracle_lib, 16, 6, 4, 50)
    assert sum(q >= 1 << 50 for q in primes) >= 1 and all(q < 1 << 51 for q in primes)
    with pytest.raises(RuntimeError, match=r"exceeds 2\^50"):
        Engine(_lib=product_lib, scale_bits=50, seed=1, **kw)
    assert all(q < 1 << 50 for q in _chain(product_lib, 16, 6, 4, 49))
    g = Engine(_lib=product_lib, scale_bits=49, seed=1, **kw)
    try:
        assert g.primes == _chain(product_lib, 16, 6, 4, 49) and g.max_level == 6
    finally:
        _drop(g)
